"""Faulty-network cluster simulation over every step entry point.

C clusters of N nodes; node i of cluster c is group c * N + i, sits in slot i
and has self_slot = i (the layout of tests/test_gpu_vote.Cluster).  Every group
carries every row with meaning at once: the follower rows and the term-run log,
the Votes masks, the timers, the configuration masks and ConfState, and the
leader half (Progress words, Match / Next / PendingSnapshot, Inflights rings,
first_index / snap_index, lead_transferee, the ReadIndex queue rows,
uncommitted_size / pending_conf_index).  Membership is static.

The per-node model composes what exists and restates nothing: vote_model /
follower_model nodes (term, state, vote, lead, log, commit), snapshot_model
(restore, compaction), tick_model.Model (timers, CheckQuorum, beats) and the C
oracle through oracle/orc.py for the leader half (progress_step, propose,
become_leader).  `World` keeps the rows the models share in step.

The simulation (`Sim`) is written against a backend with one method per entry
point.  `ModelBackend` runs the models alone; tests/test_gpu_cluster.py
subclasses it to run the engine beside them.  The step functions are
parameters of `ModelBackend`, so a negative control can swap one in.  This
module imports no torch.

The network: a seeded multiset of in-flight messages per run; per message a
drop probability, a duplication probability and a delay of 0..D rounds (the
delay reorders); per cluster at most one node cut off in both directions for
ET..4*ET rounds.  After `fault_rounds` the network is perfect for
`heal_rounds`.

Host duties the simulation relies on (include/etcd_quorum.h).  Each round is
one qe_tick; the deliveries due are grouped into whole-batch calls carrying at
most one message per group (qe_progress_step: one per slot and group).

  H1  QE_TICK_HUP -> QE_VMSG_HUP to qe_vote_step (qe_tick step 2; "After a
      QE_VR_WON" chain at qe_vote_step).
  H2  QE_TICK_BEAT -> one MsgHeartbeat{Term, Commit: hb_commit[s]} per slot of
      hb_sent (qe_tick step 3, qe_heartbeat).
  H3  QE_TICK_STEPDOWN -> the host stores lead = none (0xFF) in qe_follower.lead:
      becomeFollower(r.Term, None) (raft.go:686-693) clears r.lead, qe_tick has
      no access to that row.  (The header was silent; it says so now.)
  H4  MsgApp / MsgHeartbeat -> qe_follower_step; MsgVote / MsgPreVote / their
      responses / MsgHup -> qe_vote_step; MsgSnap -> qe_snapshot_step;
      VoteOut.elected -> qe_become_leader with QE_BL_BCAST; client proposals at
      current leaders -> qe_propose.
  H5  The events row of a call goes into the next qe_tick (ticks = 0 here,
      "events[g] ... applied before the tick").
  H6  Step's preamble for MsgAppResp / MsgHeartbeatResp is the host's
      (qe_peer_msgs carries no term):
        lower term          ignored (raft.go:883-919: neither MsgApp nor
                            MsgHeartbeat nor MsgPreVote)      -> "resp_lower_term"
        receiver not leader ignored (stepFollower / stepCandidate have no arm
                            for them, raft.go:1376-1473)       -> "resp_not_leader"
        higher term         delivered to qe_vote_step as a QE_VMSG_VOTE_RESP of
                            that term with QE_VMF_REJECT: becomeFollower(m.Term,
                            None) runs on the device (raft.go:864-881, the same
                            transition for every response type) and
                            QE_VR_STEPPED_DOWN comes back      -> "resp_higher_term"
                            (counted, not discarded)
  H7  A send reported by a `sent` mask becomes one MsgApp{Index, LogTerm,
      Entries (Index, lastIndex], Commit: committed after the call}, cut to
      QE_MAX_MSG_RUNS term runs.  Index is msg_index for qe_progress_step (the
      sends of one round to one peer are coalesced into the first: msg_count
      above 1 adds no message); for qe_propose / qe_become_leader it is Next - 1
      of a probing peer after the call and Next - 1 before the call of a
      replicating one (max_ents = 0: one MsgApp takes everything).  A bit of
      `snap` becomes MsgSnap{snap_index, term(snap_index), the ConfState}.
  H8  QE_FR_APP_ACCEPT / QE_FR_APP_STALE -> MsgAppResp{Index: resp_index};
      QE_FR_APP_REJECT -> MsgAppResp{Index, Reject, RejectHint, LogTerm};
      QE_FR_HEARTBEAT_RESP -> MsgHeartbeatResp; QE_FR_LOWER_TERM_RESP ->
      MsgAppResp{} at the receiver's term; QE_SR_STALE / NOT_MEMBER /
      FAST_FORWARD / RESTORED -> MsgAppResp{Index: resp_index}; each carries the
      receiver's term after the step.
  H9  QE_FR_RUNS_FULL / QE_BL_RUNS_FULL -> qe_compact at min(applied, committed)
      with applied = committed (a snapshot is created at the same index), then
      the same message once more.  A MsgApp refused twice is dropped
      -> "runs_full_twice"; qe_become_leader refused twice fails the run.
  H10 Nodes compact at random, at committed, creating the snapshot there.
  H11 The transport reports every MsgSnap it carried to the sender as a local
      MsgSnapStatus (node.ReportSnapshot, raft.go:1310-1331): delivered ->
      QE_MSG_SNAP_STATUS, lost -> QE_MSG_SNAP_STATUS_REJECT.  Without it a
      peer whose MsgSnap was lost stays in StateSnapshot, paused, for ever.  A
      local message has term 0 and passes Step's preamble; a sender that no
      longer leads ignores it (no arm)               -> "snap_status_not_leader"

Deliveries the host layer discards on its own decision are exactly the kinds
"resp_lower_term", "resp_not_leader", "snap_status_not_leader" and
"runs_full_twice"; `Sim.discards` counts them, any other undeliverable message
raises.  Losses of the simulated network ("net_drop", "net_cut") are counted
apart in `Sim.net`.

qe_progress_send, qe_read_index and MsgTimeoutNow are not driven: every send
the reference makes is made inside the step entry points, and no leadership
transfer or read request is issued.  The ReadIndex queue rows are resident,
empty, and compared like every other row.
"""
import copy
from collections import Counter

import numpy as np

from oracle import orc
from tests import follower_model as fm
from tests import snapshot_model as sm
from tests import tick_model as tm
from tests import vote_model as vm

NONE = fm.NONE_SLOT
PR_PROBE, PR_REPLICATE, PR_SNAPSHOT = 0, 1, 2
MSG_APP_RESP, MSG_APP_RESP_REJECT, MSG_HEARTBEAT_RESP = 1, 2, 3
BL_LEADER, BL_RUNS_FULL = 1, 3
MSG_RUNS = fm.MAX_MSG_RUNS
MSG_SNAP_STATUS, MSG_SNAP_STATUS_REJECT = 4, 5
HOST_DISCARDS = ("resp_lower_term", "resp_not_leader", "snap_status_not_leader", "runs_full_twice")


class Params:
    """One run's shape and schedule."""

    def __init__(self, N, C, R, F, ring16=False, flags=0, goff=0, base=0, learner=False, seed=1,
                 fault_rounds=60, heal_rounds=30, p_drop=0.08, p_dup=0.05, D=2, p_cut=0.15,
                 p_prop=0.5, p_compact=0.04, ET=4):
        self.N, self.C, self.R, self.F, self.ring16, self.flags = N, C, R, F, ring16, flags
        self.goff, self.base, self.learner, self.seed = goff, base, learner, seed
        self.fault_rounds, self.heal_rounds = fault_rounds, heal_rounds
        self.p_drop, self.p_dup, self.D, self.p_cut = p_drop, p_dup, D, p_cut
        self.p_prop, self.p_compact, self.ET = p_prop, p_compact, ET
        self.G = N * C
        self.stride = self.G + 3  # pad columns after every [.][stride] row

    def but(self, **kw):
        p = copy.copy(self)
        p.__dict__.update(kw)
        p.G = p.N * p.C
        p.stride = p.G + 3
        return p


class World:
    """The composed model of one batch and the rows its parts share."""

    def __init__(self, p):
        self.p = p
        G, N, st = p.G, p.N, p.stride
        full = (1 << N) - 1
        self.inc = full & ~(1 << (N - 1)) if p.learner else full
        self.learner = full & ~self.inc
        b = p.base
        ents = [(b, 1 if b else 0), (b + 1, 1), (b + 2, 1)]
        self.nodes = [vm.Node(ents, committed=b + 2, term=1, self_slot=g % N, inc=self.inc,
                              tracked=full) for g in range(G)]
        conf = sm.Conf(N, self.inc, 0, self.learner, ids=[s + 1 for s in range(N)])
        self.confs = [conf] * G
        self.snap_index = [b] * G
        cq = bool(p.flags & vm.VOTE_CHECK_QUORUM)
        self.tm = m = tm.Model(G, N, p.ET, 1, cq, seed=p.seed, goff=p.goff, stride=st)
        md = orc.mask_dtype(N)
        self.pb = pb = orc.ProgressBatch(G, N, p.F, p.R, stride=st, max_ents=0)
        pb.ring16 = bool(p.ring16)
        pb.inc = np.full(G, self.inc, md)
        pb.tracked = np.full(G, full, md)
        pb.self_slot = np.array([g % N for g in range(G)], np.uint8)
        pb.lead_transferee = np.full(G, NONE, np.uint8)
        pb.snap_index = np.zeros(G, np.uint64)
        pb.track_reads()
        pb.next[:] = b + 3
        self.pci = np.zeros(G, np.uint64)
        self.unc = np.zeros(G, np.uint64)
        # the tick model reads the leader rows where they live
        m.peer, m.match, m.committed = pb.pw, pb.match, pb.committed
        m.lead_transferee, m.self_slot = pb.lead_transferee, pb.self_slot
        m.inc, m.tracked = pb.inc, pb.tracked
        m.read_head, m.read_count = pb.read_head, pb.read_count
        rt = np.random.default_rng(p.seed).integers(p.ET, 2 * p.ET, G)
        m.rt[:] = rt  # staggered first timeouts, as Cluster
        for g in range(G):
            self.push(g)

    def push(self, g):
        """nodes[g] -> the rows the oracle and the tick model read."""
        n, pb, st = self.nodes[g], self.pb, self.p.stride
        pb.committed[g], pb.last_index[g] = n.committed, n.last_index()
        pb.first_index[g] = n.ents[0][0] + 1
        pb.snap_index[g] = self.snap_index[g]
        pb.lead_transferee[g] = n.transferee
        pb.run_count[g] = len(n.runs)
        for r, (f, t) in enumerate(n.runs):
            pb.run_first[r * st + g], pb.run_term[r * st + g] = f, t
        self.tm.state[g] = n.state

    def pull(self, g):
        """The oracle's rows of group g (a leader) -> nodes[g]: entries the
        leader appended take its term; the oracle's run table must be the
        node's."""
        n, pb, st = copy.deepcopy(self.nodes[g]), self.pb, self.p.stride
        last, new_last = n.last_index(), int(pb.last_index[g])
        assert new_last >= last
        if new_last > last:
            if n.runs[-1][1] != n.term:
                n.runs.append((last + 1, n.term))
            n.ents += [(i, n.term) for i in range(last + 1, new_last + 1)]
        n.committed = int(pb.committed[g])
        n.transferee = int(pb.lead_transferee[g])
        n.check()
        got = [(int(pb.run_first[r * st + g]), int(pb.run_term[r * st + g]))
               for r in range(int(pb.run_count[g]))]
        assert got == n.runs, ("the oracle's run table left the node's", g, got, n.runs)
        self.nodes[g] = n

    def snode(self, g):
        return sm.SNode(self.nodes[g], self.confs[g], g % self.p.N, self.snap_index[g])

    def put_snode(self, g, sn):
        self.nodes[g], self.confs[g], self.snap_index[g] = sn.node, sn.conf, sn.snap_index
        self.push(g)

    def pstate(self, g, s):
        return int(self.pb.pw[s * self.p.stride + g]) & 3

    def icount(self, g, s):
        return (int(self.pb.pw[s * self.p.stride + g]) >> 16) & 0xFF


def node_view(n):
    return {"term": n.term, "state": n.state, "committed": n.committed,
            "first_index": n.ents[0][0] + 1, "last_index": n.last_index(), "runs": list(n.runs)}


class ModelBackend:
    """One method per entry point, on the models alone.  Each returns the
    model's outputs; the state is `self.w`."""

    WORLD = World  # a subclass may compose another initial state (tests/trace_cluster.py)

    def __init__(self, p, vote_step=vm.step, follower_step=fm.step):
        self.p, self.w = p, self.WORLD(p)
        self.vote_step_fn, self.follower_step_fn = vote_step, follower_step
        self.calls = Counter()

    # ---- qe_tick ----
    def tick(self, events, ticks):
        """events: None or uint8[G] (the events row of the call before)."""
        w = self.w
        self.calls["tick"] += 1
        out = w.tm.tick(events, ticks=ticks)
        for g in np.flatnonzero(out.action & tm.STEPDOWN):
            n = w.nodes[g] = copy.deepcopy(w.nodes[g])
            n.state, n.transferee = fm.ST_FOLLOWER, NONE
        return out

    def clear_lead(self, groups):
        """H3: the host's write after QE_TICK_STEPDOWN."""
        for g in groups:
            n = self.w.nodes[g] = copy.deepcopy(self.w.nodes[g])
            n.lead = NONE

    # ---- qe_vote_step ----
    def vote(self, msgs):
        w, p = self.w, self.p
        self.calls["vote"] += 1
        outs = []
        for g, m in enumerate(msgs):
            if m.type == vm.VMSG_NONE:
                outs.append({"result": vm.VR_NONE, "events": 0, "elected": 0})
                continue
            w.nodes[g].elapsed = int(w.tm.ee[g])
            n2, o = self.vote_step_fn(w.nodes[g], m, p.flags, p.N, p.ET)
            w.nodes[g] = n2
            w.push(g)
            outs.append(o)
        return outs

    # ---- qe_follower_step ----
    def follow(self, msgs):
        w, p = self.w, self.p
        self.calls["follow"] += 1
        outs = []
        for g, m in enumerate(msgs):
            if m.type == fm.LMSG_NONE:
                outs.append({"result": fm.FR_NONE, "events": 0})
                continue
            n2, o = self.follower_step_fn(w.nodes[g], m, p.flags & 3, p.N, p.R)
            w.nodes[g] = n2
            w.push(g)
            outs.append(o)
        return outs

    # ---- qe_snapshot_step ----
    def snap(self, msgs):
        w, p = self.w, self.p
        self.calls["snap"] += 1
        outs = []
        for g, m in enumerate(msgs):
            if m.type == sm.SMSG_NONE:
                outs.append({"result": sm.SR_NONE, "events": 0})
                continue
            sn, o = sm.step(w.snode(g), m, p.N, p.R)
            w.put_snode(g, sn)
            outs.append(o)
        return outs

    # ---- qe_compact ----
    def compact(self, reqs):
        """reqs: (ci, si, applied) per group, (0, 0, 0) = none."""
        w = self.w
        self.calls["compact"] += 1
        outs = []
        for g, (ci, si, ap) in enumerate(reqs):
            if not ci and not si:
                outs.append({"result": sm.CP_NONE})
                continue
            sn, o = sm.compact(w.snode(g), ci, si, ap)
            w.put_snode(g, sn)
            outs.append(o)
        return outs

    # ---- qe_become_leader (QE_BL_BCAST) ----
    def become_leader(self, elected):
        w = self.w
        self.calls["become_leader"] += 1
        term = np.array([n.term for n in w.nodes], np.uint64)
        o = orc.become_leader(w.pb, term, elected, bcast=True)
        for g in np.flatnonzero(o.result == BL_LEADER):
            w.pci[g], w.unc[g] = o.pending_conf_index[g], o.uncommitted_size[g]
            w.pull(g)
        return o

    # ---- qe_propose ----
    def propose(self, num_entries):
        w = self.w
        self.calls["propose"] += 1
        o = orc.propose(w.pb, num_entries, pending_conf_index=w.pci, uncommitted_size=w.unc)
        for g in np.flatnonzero(num_entries):
            w.pull(g)
        return o

    # ---- qe_progress_step ----
    def progress_step(self, mtype, mindex, mhint, mlogterm):
        w, st = self.w, self.p.stride
        self.calls["progress_step"] += 1
        o = orc.progress_step(w.pb, mtype, mindex, mhint, mlogterm, threads=1)
        for g in np.flatnonzero(mtype.reshape(self.p.N, st)[:, : self.p.G].any(0)):
            w.pull(g)
        return o

    def view(self):
        return [node_view(n) for n in self.w.nodes]


# ---------------------------------------------------------------------------
# The invariants
# ---------------------------------------------------------------------------
class InvariantError(AssertionError):
    pass


def term_at(v, i):
    """term(i) on a view's run table, i in [dummy, last_index]."""
    t = None
    for f, rt in v["runs"]:
        if f <= i:
            t = rt
    return t


def terms_of(v, lo, hi):
    """The terms of [lo, hi] (inside the log) as a list."""
    out, runs = [], v["runs"]
    r = 0
    for i in range(lo, hi + 1):
        while r + 1 < len(runs) and runs[r + 1][0] <= i:
            r += 1
        out.append(runs[r][1])
    return out


class Invariants:
    """check(view) after every round, view = the plain per-node state (term,
    state, committed, first_index, last_index, the run table):
      Election Safety   at most one node ever leads a (cluster, term);
      Monotonicity      term and committed never decrease; while a node leads
                        a term its last_index does not shrink and its term's
                        run does not move;
      Log Matching      two logs that agree at an index agree at every lower
                        index both hold; and (a corollary: every log is a
                        prefix-by-prefix copy of leaders' logs) terms never
                        decrease along a log;
      State Machine Safety / Leader Completeness
                        a per-cluster record index -> term of everything any
                        node reported committed; no node's committed prefix may
                        contradict it (an UNcommitted tail of a deposed leader
                        legally differs until qe_follower_step truncates it);
                        a new leader's log holds the record's last entry, or
                        has compacted past it with a matching snapshot term.
    converged(view) after the heal: one leader per cluster, at the highest term;
    every committed equals its last_index; the run tables agree."""

    def __init__(self, C, N):
        self.C, self.N = C, N
        self.leaders = {}              # (cluster, term) -> slot
        self.prev = None
        self.record = [dict() for _ in range(C)]  # index -> term of everything reported committed
        self.reported = [0] * (C * N)  # the highest index a node reported committed
        self.lead_log = {}             # (cluster, term) -> (last_index, its term run's first index)

    def fail(self, what, *a):
        raise InvariantError(what + ": " + repr(a))

    def check(self, view):
        N = self.N
        for g, v in enumerate(view):
            c, dummy = g // N, v["first_index"] - 1
            runs = v["runs"]
            if not (runs[0][0] == dummy <= v["committed"] <= v["last_index"]):
                self.fail("log bounds", g, v)
            # (a corollary of Log Matching: every log is a leader's, term by term)
            if any(runs[k][1] > runs[k + 1][1] or runs[k][0] >= runs[k + 1][0]
                   for k in range(len(runs) - 1)):
                self.fail("Log Matching: terms decrease along a log", g, runs)
            if self.prev is not None:
                q = self.prev[g]
                if v["term"] < q["term"] or v["committed"] < q["committed"]:
                    self.fail("Monotonicity", g, q, v)
            if v["state"] == fm.ST_LEADER:
                key = (c, v["term"])
                new = key not in self.lead_log
                if self.leaders.setdefault(key, g % N) != g % N:
                    self.fail("Election Safety", key, self.leaders[key], g % N)
                if runs[-1][1] != v["term"]:
                    self.fail("a leader's last run is not its term's", g, v)
                first = runs[-1][0] if len(runs) > 1 or dummy < runs[-1][0] else None
                if not new and key in self.lead_log:
                    last0, first0 = self.lead_log[key]
                    if v["last_index"] < last0 or (first is not None and first0 is not None and
                                                   first != first0 and first != dummy):
                        self.fail("Monotonicity: a leader's own-term log was truncated", g, v)
                    first = first if first is not None else first0
                self.lead_log[key] = (v["last_index"], first)
                if new:
                    self.leader_completeness(c, g, v)
        for c in range(self.C):
            vs = view[c * N:(c + 1) * N]
            self.log_matching(c, vs)
            self.commit_safety(c, vs)
        self.prev = view

    def log_matching(self, c, vs):
        for a in range(self.N):
            for b in range(a + 1, self.N):
                lo = max(vs[a]["first_index"], vs[b]["first_index"]) - 1
                hi = min(vs[a]["last_index"], vs[b]["last_index"])
                if lo > hi:
                    continue
                ta, tb = terms_of(vs[a], lo, hi), terms_of(vs[b], lo, hi)
                eq = [x == y for x, y in zip(ta, tb)]
                if True in eq:
                    top = len(eq) - 1 - eq[::-1].index(True)
                    if not all(eq[:top]):
                        self.fail("Log Matching", c, a, b, lo, ta, tb)

    def commit_safety(self, c, vs):
        rec = self.record[c]
        for i, v in enumerate(vs):
            g = c * self.N + i
            dummy = v["first_index"] - 1
            lo = max(self.reported[g] + 1, dummy)
            if lo <= v["committed"]:
                for idx, t in zip(range(lo, v["committed"] + 1), terms_of(v, lo, v["committed"])):
                    if rec.setdefault(idx, t) != t:
                        self.fail("State Machine Safety", c, i, idx, t, rec[idx])
            self.reported[g] = max(self.reported[g], v["committed"])
        if not rec:
            return
        low = min(v["first_index"] - 1 for v in vs)
        for idx in [k for k in rec if k < low]:
            del rec[idx]
        top = max(rec)
        for i, v in enumerate(vs):
            # (up to its commit index: an uncommitted tail of a deposed leader may
            # differ until qe_follower_step truncates it)
            lo, hi = max(v["first_index"] - 1, low), min(v["committed"], top)
            if lo <= hi:
                for idx, t in zip(range(lo, hi + 1), terms_of(v, lo, hi)):
                    if idx in rec and rec[idx] != t:
                        self.fail("State Machine Safety: a log contradicts the record", c, i,
                                  idx, t, rec[idx])

    def leader_completeness(self, c, g, v):
        rec = self.record[c]
        if not rec:
            return
        top, dummy = max(rec), v["first_index"] - 1
        if top > v["last_index"]:
            self.fail("Leader Completeness: the record's last entry is missing", c, g, top, v)
        if top >= dummy:
            if term_at(v, top) != rec[top]:
                self.fail("Leader Completeness", c, g, top, rec[top], v)
        elif dummy in rec and rec[dummy] != v["runs"][0][1]:
            self.fail("Leader Completeness: snapshot term", c, g, v)

    def converged(self, view):
        N = self.N
        for c in range(self.C):
            vs = view[c * N:(c + 1) * N]
            lead = [v for v in vs if v["state"] == fm.ST_LEADER]
            if len(lead) != 1 or lead[0]["term"] != max(v["term"] for v in vs):
                self.fail("Convergence: not one leader at the highest term", c, vs)
            for v in vs:
                if v["committed"] != lead[0]["last_index"]:
                    self.fail("Convergence: committed", c, v, lead[0])
            for v in vs:
                lo, hi = max(v["first_index"], lead[0]["first_index"]) - 1, v["last_index"]
                if hi != lead[0]["last_index"] or terms_of(v, lo, hi) != terms_of(lead[0], lo, hi):
                    self.fail("Convergence: run tables", c, v, lead[0])


# ---------------------------------------------------------------------------
# The simulation
# ---------------------------------------------------------------------------
F_CLS, V_CLS, S_CLS, R_CLS = "follow", "vote", "snap", "resp"


class Net:
    """A message in flight."""
    __slots__ = ("due", "seq", "cls", "to", "frm", "term", "m")

    def __init__(self, due, seq, cls, to, frm, term, m):
        self.due, self.seq, self.cls, self.to, self.frm, self.term, self.m = \
            due, seq, cls, to, frm, term, m


class Sim:
    def __init__(self, p, backend, stale_resp_ok=False):
        self.p, self.be, self.w = p, backend, backend.w
        self.rng = np.random.default_rng(p.seed * 7919 + 13)
        self.inv = Invariants(p.C, p.N)
        self.net_q, self.seq, self.round_no = [], 0, 0
        self.cut = [None] * p.C       # (slot, until round)
        self.events = None
        self.cov, self.discards, self.net = Counter(), Counter(), Counter()
        self.led = set()              # groups that have led
        self.stepped_down = set()     # groups qe_tick deposed
        self.lead_slots = [set() for _ in range(p.C)]
        self.stale_resp_ok = stale_resp_ok  # negative control: H6's first rule off
        self.faulty = True

    # ---- the network ----
    def send(self, cls, frm_g, to_g, term, m):
        p, rng = self.p, self.rng
        copies = 1
        if self.faulty:
            if rng.random() < p.p_drop:
                self.net["net_drop"] += 1
                if cls == S_CLS:
                    self.snap_status(frm_g, to_g % p.N, False)
                return
            if rng.random() < p.p_dup:
                copies = 2
        for _ in range(copies):
            d = int(rng.integers(0, p.D + 1)) if self.faulty else 0
            self.seq += 1
            self.net_q.append(Net(self.round_no + d, self.seq, cls, to_g, frm_g % p.N, term,
                                  copy.copy(m)))

    def snap_status(self, leader_g, slot, ok):
        """H11: a local message, no network in between."""
        self.seq += 1
        # (a success is known a round later: the MsgAppResp may overtake it)
        self.net_q.append(Net(self.round_no + int(ok), self.seq, R_CLS, leader_g, slot, None,
                              (MSG_SNAP_STATUS if ok else MSG_SNAP_STATUS_REJECT, 0, 0, 0)))

    def is_cut(self, g):
        c = self.cut[g // self.p.N]
        return c is not None and c[0] == g % self.p.N

    def settle(self, events):
        """H5."""
        if np.any(events):
            self.be.tick(np.asarray(events, np.uint8), 0)

    # ---- what a leader-side call sent (H7) ----
    def emit(self, g, sent, snap, index_of):
        w, p = self.w, self.p
        n, base = w.nodes[g], g - g % p.N
        for s in range(p.N):
            if snap >> s & 1:
                si = w.snap_index[g]
                m = sm.SMsg(sm.SMSG_SNAP, g % p.N, n.term, si, n.log_term(si), w.inc, 0, w.learner)
                self.send(S_CLS, g, base + s, n.term, m)
            elif sent >> s & 1:
                idx = index_of(s)
                runs = []
                for _, t in n.ents[idx - n.ents[0][0] + 1:]:
                    if runs and runs[-1][1] == t:
                        runs[-1][0] += 1
                    elif len(runs) < MSG_RUNS:
                        runs.append([1, t])
                    else:
                        break
                m = fm.Msg(fm.LMSG_APP, g % p.N, n.term, idx, n.log_term(idx), n.committed, runs)
                self.send(F_CLS, g, base + s, n.term, m)

    def next_index_rule(self, g, next_before):
        w, st = self.w, self.p.stride

        def index_of(s):
            if w.pstate(g, s) == PR_PROBE:
                return int(w.pb.next[s * st + g]) - 1
            return int(next_before[s * st + g]) - 1
        return index_of

    # ---- the calls ----
    def do_vote(self, msgs):
        p, w = self.p, self.w
        outs = self.be.vote(msgs)
        elected = np.array([o["elected"] for o in outs], np.uint8)
        for g, o in enumerate(outs):
            r = o["result"]
            if r == vm.VR_NONE:
                continue
            assert r < vm.VR_REFUSED, (g, msgs[g], o)
            self.cov[vm.VR_NAMES[r]] += 1
            n, m = w.nodes[g], msgs[g]
            if r in (vm.VR_CAMPAIGN_VOTE, vm.VR_CAMPAIGN_PREVOTE):
                if g in self.stepped_down:
                    self.cov["stepdown_then_campaign"] += 1
                ty = vm.VMSG_VOTE if r == vm.VR_CAMPAIGN_VOTE else vm.VMSG_PREVOTE
                for s in range(p.N):
                    if o["req_to"] >> s & 1:
                        self.send(V_CLS, g, g - g % p.N + s, o["resp_term"],
                                  vm.Msg(ty, g % p.N, o["resp_term"], n.last_index(),
                                         o["req_log_term"]))
            elif r in (vm.VR_GRANT, vm.VR_REJECT) and m.type in (vm.VMSG_VOTE, vm.VMSG_PREVOTE):
                self.send(V_CLS, g, g - g % p.N + m.frm, o["resp_term"],
                          vm.Msg(m.type + 2, g % p.N, o["resp_term"],
                                 flags=vm.VMF_REJECT if r == vm.VR_REJECT else 0))
        self.settle([o["events"] for o in outs])
        if elected.any():
            self.do_become_leader(elected)

    def do_become_leader(self, elected, retried=False):
        p, w, st = self.p, self.w, self.p.stride
        live = [g for g in np.flatnonzero(elected)
                if g in self.led and any(w.icount(g, s) for s in range(p.N))]
        o = self.be.become_leader(elected)
        full = o.result == BL_RUNS_FULL
        for g in np.flatnonzero(o.result == BL_LEADER):
            key = (g // p.N, w.nodes[g].term)  # as Cluster.leaders: recorded as it happens
            if self.inv.leaders.setdefault(key, g % p.N) != g % p.N:
                self.inv.fail("Election Safety", key, self.inv.leaders[key], g % p.N)
            self.led.add(g)
            self.stepped_down.discard(g)
            self.lead_slots[g // p.N].add(g % p.N)
            if g in live:
                self.cov["releader_live_rings"] += 1
            self.emit(g, int(o.sent[g]), int(o.snap[g]),
                      lambda s, g=g: int(w.pb.next[s * st + g]) - 1)
        assert set(np.unique(o.result)) <= {0, BL_LEADER, BL_RUNS_FULL}, o.result
        if full.any():
            assert not retried, "qe_become_leader refused twice (QE_BL_RUNS_FULL)"
            self.do_compact({g: w.nodes[g].committed for g in np.flatnonzero(full)})
            self.cov["bl_runs_full_retry"] += 1
            self.do_become_leader(full.astype(np.uint8), retried=True)

    def do_compact(self, at):
        """at: group -> index (H9, H10)."""
        w = self.w
        reqs = [(0, 0, 0)] * self.p.G
        for g, ci in at.items():
            reqs[g] = (ci, ci, w.nodes[g].committed)
        for g, o in enumerate(self.be.compact(reqs)):
            if o["result"] & sm.CP_COMPACTED and o["result"] < sm.CP_REFUSED:
                self.cov["CP_COMPACTED"] += 1

    def do_follow(self, msgs, retried=False):
        p, w = self.p, self.w
        last_before = [n.last_index() for n in w.nodes]
        outs = self.be.follow(msgs)
        again = {}
        for g, o in enumerate(outs):
            r = o["result"]
            if r == fm.FR_NONE:
                continue
            self.cov[fm.FR_NAMES[r]] += 1
            n, m = w.nodes[g], msgs[g]
            to = g - g % p.N + m.frm
            if r == fm.FR_RUNS_FULL:
                again[g] = m
                continue
            assert r < fm.FR_REFUSED, (g, vars(m), o)
            if retried and r == fm.FR_APP_ACCEPT:
                self.cov["runs_full_retry_ok"] += 1
            if r in (fm.FR_APP_ACCEPT, fm.FR_APP_STALE):
                if r == fm.FR_APP_ACCEPT and 0 < o["append_from"] <= last_before[g]:
                    self.cov["fr_truncate"] += 1
                self.send(R_CLS, g, to, n.term, (MSG_APP_RESP, o["resp_index"], 0, 0))
            elif r == fm.FR_APP_REJECT:
                self.send(R_CLS, g, to, n.term,
                          (MSG_APP_RESP_REJECT, o["resp_index"], o["reject_hint"],
                           o["resp_log_term"]))
            elif r == fm.FR_HEARTBEAT_RESP:
                self.send(R_CLS, g, to, n.term, (MSG_HEARTBEAT_RESP, 0, 0, 0))
            elif r == fm.FR_LOWER_TERM_RESP:
                self.send(R_CLS, g, to, n.term, (MSG_APP_RESP, 0, 0, 0))
        self.settle([o["events"] for o in outs])
        if again:
            if retried:
                self.discards["runs_full_twice"] += len(again)
                return
            self.do_compact({g: w.nodes[g].committed for g in again})
            msgs = [again.get(g, fm.Msg()) for g in range(p.G)]
            self.do_follow(msgs, retried=True)

    def do_snap(self, msgs):
        p, w = self.p, self.w
        outs = self.be.snap(msgs)
        for g, o in enumerate(outs):
            r = o["result"]
            if r == sm.SR_NONE:
                continue
            assert r < sm.SR_REFUSED, (g, vars(msgs[g]), o)
            self.cov[sm.SR_NAMES[r]] += 1
            self.snap_status(g - g % p.N + msgs[g].frm, g % p.N, True)
            if r != sm.SR_IGNORED:
                self.send(R_CLS, g, g - g % p.N + msgs[g].frm, w.nodes[g].term,
                          (MSG_APP_RESP, o["resp_index"], 0, 0))
        self.settle([o["events"] for o in outs])

    def do_progress(self, items):
        """items: (group, slot, (type, index, hint, logterm))."""
        p, w, st = self.p, self.w, self.p.stride
        n = p.N * st
        mtype, mindex = np.zeros(n, np.uint8), np.zeros(n, np.uint64)
        mhint, mlog = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        for g, s, (t, i, h, lt) in items:
            k = s * st + g
            mtype[k], mindex[k], mhint[k], mlog[k] = t, i, h, lt
        nxt0, pw0, com0 = w.pb.next.copy(), w.pb.pw.copy(), w.pb.committed.copy()
        o = self.be.progress_step(mtype, mindex, mhint, mlog)
        for g, s, (t, _, _, _) in items:
            k = s * st + g
            if t == MSG_APP_RESP_REJECT and w.pb.next[k] < nxt0[k]:
                self.cov["next_down"] += 1
            if t == MSG_APP_RESP and pw0[k] & 3 == PR_SNAPSHOT and w.pstate(g, s) == PR_REPLICATE:
                self.cov["snapshot_probe_replicate"] += 1
        for g in sorted({g for g, _, _ in items}):
            if w.pb.committed[g] > com0[g]:
                self.cov["commit_advance"] += 1
            mi = o.msg_index
            self.emit(g, int(o.sent[g]), int(o.snap[g]), lambda s, g=g: int(mi[s * st + g]))

    def do_propose(self, ne):
        p, w, st = self.p, self.w, self.p.stride
        nxt0 = w.pb.next.copy()
        o = self.be.propose(ne)
        for g in np.flatnonzero(ne):
            assert o.result[g] == 1, (g, o.result[g])  # QE_PROP_OK
            self.cov["proposals"] += 1
            sent = int(o.sent[g]) | int(o.snap[g])
            for s in range(p.N):
                if s != g % p.N and not sent >> s & 1 and w.pstate(g, s) == PR_REPLICATE and \
                        w.icount(g, s) == p.F and w.pb.next[s * st + g] <= w.pb.last_index[g]:
                    self.cov["withheld_inflights_full"] += 1
            self.emit(g, int(o.sent[g]), int(o.snap[g]), self.next_index_rule(g, nxt0))

    # ---- one round ----
    def deliver(self, queue):
        """Whole-batch calls over the messages due, at most one per group and
        call (responses: one per slot and group), in sending order."""
        p, w = self.p, self.w
        while queue:
            wave, rest, blocked = {}, [], set()
            for x in queue:
                g = x.to
                if g not in wave and g not in blocked:
                    wave[g] = [x]
                elif g in wave and g not in blocked and x.cls == R_CLS and \
                        wave[g][0].cls == R_CLS and all(y.frm != x.frm for y in wave[g]):
                    wave[g].append(x)
                else:
                    blocked.add(g)
                    rest.append(x)
            mark = len(self.net_q)
            fmsgs = {g: xs[0].m for g, xs in wave.items() if xs[0].cls == F_CLS}
            smsgs = {g: xs[0].m for g, xs in wave.items() if xs[0].cls == S_CLS}
            vmsgs = {g: xs[0].m for g, xs in wave.items() if xs[0].cls == V_CLS}
            items, late = [], []
            for g, xs in wave.items():
                if xs[0].cls != R_CLS:
                    continue
                n = w.nodes[g]
                for x in xs:  # H6
                    if x.term is None:  # H11
                        if n.state == fm.ST_LEADER:
                            items.append((g, x.frm, x.m))
                        else:
                            self.discards["snap_status_not_leader"] += 1
                    elif x.term < n.term and not (self.stale_resp_ok and n.state == fm.ST_LEADER):
                        self.discards["resp_lower_term"] += 1
                    elif x.term > n.term:
                        if g in vmsgs:
                            late.append(x)
                        else:
                            self.cov["resp_higher_term"] += 1
                            vmsgs[g] = vm.Msg(vm.VMSG_VOTE_RESP, x.frm, x.term,
                                              flags=vm.VMF_REJECT)
                    elif n.state != fm.ST_LEADER:
                        self.discards["resp_not_leader"] += 1
                    else:
                        items.append((g, x.frm, x.m))
            if fmsgs:
                self.do_follow([fmsgs.get(g, fm.Msg()) for g in range(p.G)])
            if smsgs:
                self.do_snap([smsgs.get(g, sm.SMsg()) for g in range(p.G)])
            if items:
                self.do_progress(items)
            if vmsgs:
                self.do_vote([vmsgs.get(g, vm.Msg()) for g in range(p.G)])
            # what the calls sent with no delay is due in this round too
            new = [x for x in self.net_q[mark:] if x.due <= self.round_no]
            self.net_q[mark:] = [x for x in self.net_q[mark:] if x.due > self.round_no]
            queue = sorted(rest + late + self.arrived(new), key=lambda x: x.seq)

    def arrived(self, xs):
        """The messages of xs that no cut swallows."""
        keep = []
        for x in xs:
            if self.is_cut(x.to) or self.is_cut(x.to - x.to % self.p.N + x.frm):
                self.net["net_cut"] += 1
                if x.cls == S_CLS:
                    self.snap_status(x.to - x.to % self.p.N + x.frm, x.to % self.p.N, False)
            else:
                keep.append(x)
        return keep

    def round(self):
        p, w, rng = self.p, self.w, self.rng
        self.round_no += 1
        self.faulty = self.round_no <= p.fault_rounds
        for c in range(p.C):
            if self.cut[c] is not None and (not self.faulty or self.cut[c][1] < self.round_no):
                self.cut[c] = None
            if self.faulty and self.cut[c] is None and rng.random() < p.p_cut:
                self.cut[c] = (int(rng.integers(0, p.N)),
                               self.round_no + int(rng.integers(p.ET, 4 * p.ET + 1)))
        out = self.be.tick(None, 1)
        down = [int(g) for g in np.flatnonzero(out.action & tm.STEPDOWN)]
        if down:
            self.cov["TICK_STEPDOWN"] += len(down)
            self.stepped_down |= set(down)
            self.be.clear_lead(down)  # H3
        hc = out.hb_commit.reshape(p.N, p.stride)
        for g in np.flatnonzero(out.action & tm.BEAT):  # H2
            n = w.nodes[g]
            for s in range(p.N):
                if int(out.hb_sent[g]) >> s & 1:
                    self.send(F_CLS, g, g - g % p.N + s, n.term,
                              fm.Msg(fm.LMSG_HEARTBEAT, g % p.N, n.term, commit=int(hc[s, g])))
        due = [x for x in self.net_q if x.due <= self.round_no]
        self.net_q = [x for x in self.net_q if x.due > self.round_no]
        queue = sorted(self.arrived(due), key=lambda x: x.seq)
        hups = [Net(0, 0, V_CLS, int(g), 0, 0, vm.Msg(vm.VMSG_HUP))
                for g in np.flatnonzero(out.action & tm.HUP)]  # H1
        self.deliver(hups + queue)
        ne = np.zeros(p.G, np.uint32)
        for g, n in enumerate(w.nodes):
            if n.state == fm.ST_LEADER and rng.random() < p.p_prop:
                ne[g] = int(rng.integers(1, 3))
        if ne.any():
            self.do_propose(ne)
            due = [x for x in self.net_q if x.due <= self.round_no]
            self.net_q = [x for x in self.net_q if x.due > self.round_no]
            self.deliver(sorted(self.arrived(due), key=lambda x: x.seq))
        at = {g: n.committed for g, n in enumerate(w.nodes)
              if n.committed > n.ents[0][0] and rng.random() < p.p_compact}
        if at:
            self.do_compact(at)
        view = self.be.view()
        self.inv.check(view)
        return view

    def run(self):
        p = self.p
        view = None
        for _ in range(p.fault_rounds + p.heal_rounds):
            view = self.round()
        self.inv.converged(view)
        self.finish(view)
        return self

    def finish(self, view):
        p = self.p
        for c in range(p.C):
            if len(self.lead_slots[c]) >= 2:
                self.cov["two_leaders"] += 1
            top = max(v["term"] for v in view[c * p.N:(c + 1) * p.N])
            if top >= 4:
                self.cov["term_ge_4"] += 1
            if any((c, t) not in self.inv.leaders for t in range(2, top)):
                self.cov["term_without_leader"] += 1
        assert set(self.discards) <= set(HOST_DISCARDS), self.discards

    def counters(self):
        """Everything that shows which schedule ran."""
        return {"cov": dict(self.cov), "discards": dict(self.discards), "net": dict(self.net),
                "calls": dict(self.be.calls), "leaders": len(self.inv.leaders)}


# ---------------------------------------------------------------------------
# The rows of tests/test_gpu_cluster.py and what each must meet
# ---------------------------------------------------------------------------
CQ, PV = vm.VOTE_CHECK_QUORUM, vm.VOTE_PREVOTE
ROWS = {
    # 16-bit Inflights form, cap 4; every index crosses 2^32 during the run
    "a": Params(N=3, C=66, R=4, F=4, ring16=True, flags=0, base=(1 << 32) - 5, seed=11,
                fault_rounds=40, heal_rounds=30, p_dup=0.1, p_compact=0.01),
    # 32-bit rings, cap 2, PreVote + CheckQuorum, one learner (slot 4), group_offset 2^33
    "b": Params(N=5, C=27, R=8, F=2, flags=PV | CQ, goff=1 << 33, learner=True, seed=12,
                fault_rounds=30, heal_rounds=15, p_dup=0.1),
    # less than one tile; log_runs 16 rules the 16-bit form out (it needs log_runs <= 4)
    "c": Params(N=3, C=1, R=16, F=4, flags=CQ, seed=13, fault_rounds=260, heal_rounds=15,
                p_cut=0.25, p_dup=0.2),
}

ALWAYS = ("VR_GRANT", "VR_REJECT", "VR_WON", "VR_STEPPED_DOWN", "VR_IGNORED",
          "FR_APP_ACCEPT", "FR_APP_REJECT", "FR_APP_STALE", "FR_HEARTBEAT_RESP", "fr_truncate",
          "SR_RESTORED", "CP_COMPACTED", "next_down", "snapshot_probe_replicate",
          "withheld_inflights_full", "commit_advance", "releader_live_rings", "two_leaders",
          "term_ge_4")
EITHER = (("VR_LOST", "term_without_leader"), ("SR_STALE", "SR_FAST_FORWARD"))


def required(name):
    """-> (keys that must be > 0, tuples of which one must be > 0).  Rows
    without CheckQuorum cannot meet VR_IN_LEASE (no lease) nor a QE_TICK_STEPDOWN
    (no MsgCheckQuorum); rows without flags answer no lower-term message
    (QE_FR_IGNORED instead of QE_FR_LOWER_TERM_RESP); PreVote is row b's."""
    p = ROWS[name]
    keys, either = list(ALWAYS), list(EITHER)
    if not p.flags & 3:
        # no response of a higher term is ever sent: a lower-term request or
        # MsgApp is ignored without CheckQuorum / PreVote (raft.go:883-919), and
        # QE_VR_STEPPED_DOWN is the result of a response alone
        keys.remove("VR_STEPPED_DOWN")
    if p.flags & CQ:
        keys += ["VR_IN_LEASE", "stepdown_then_campaign"]
    if p.flags & PV:
        keys.append("VR_CAMPAIGN_PREVOTE")
    either.append(("FR_LOWER_TERM_RESP", "FR_IGNORED") if p.flags & 3 else ("FR_IGNORED",))
    if name == "a":
        keys.append("runs_full_retry_ok")
    return keys, either


def missing(name, cov):
    keys, either = required(name)
    return [k for k in keys if not cov.get(k)] + [e for e in either
                                                  if not any(cov.get(k) for k in e)]
