"""tests/trace_cluster.py with the storage half of every Ready taken from
qe_ready's records: a replay that calls the note after every follower /
snapshot call, `ready` at every Ready block and `advance` right after, and
compares MustSync, the SoftState and HardState (vote included), Entries,
CommittedEntries and the Snapshot index of the record with what the reference
printed (tests/golden/ready_blocks.json).  Nothing of it comes from the
driver's own `unstable` / `applied` bookkeeping, which keeps running beside it
for the plain replay's checks.  Imports no torch.

A backend adds three methods to trace_cluster's: the note (made inside its
follower / snapshot calls), `list_ready(pending)` -> the records of the whole
batch, and `advance_ready(records)` -> their results.  `ReadyModelBackend` runs
tests/ready_model.py on the World's rows; tests/test_gpu_ready.py runs the
engine.

VOTED_FOR_1 and KNEW_A_LEADER close, by name, the gaps of the restated start states (the rule
has none): confchange_v1_remove_leader.txt restates no Vote -- every node voted
for node 1, as its first printed HardState says; in probe_and_replicate.txt the
nodes 2, 4 and 5 still knew a leader that INITIAL restates as None (their
Readies at lines 416, 427 and 433 print the SoftState "Lead:0"), so their
prev_lead starts at a slot.  Nothing else is exempt."""
import json
import os
from collections import Counter

import numpy as np

from tests import cluster_sim as cs
from tests import outbox_sim as osim
from tests import ready_model as rdm
from tests import trace_cluster as tc
from tests.trace_replay import traces

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ready_blocks.json")
# the Ready blocks of the mandatory traces: 9 + 8 + 36 + 7 + 12
BLOCKS = {"campaign.txt": 9, "campaign_learner_must_vote.txt": 8, "probe_and_replicate.txt": 36,
          "snapshot_succeed_via_app_resp.txt": 7, "confchange_v1_remove_leader.txt": 12}
assert tuple(BLOCKS) == tc.MANDATORY and sum(BLOCKS.values()) == 72
VOTED_FOR_1 = ("confchange_v1_remove_leader.txt",)
KNEW_A_LEADER = {"probe_and_replicate.txt": (2, 4, 5)}


def ready_blocks():
    with open(GOLDEN, encoding="utf-8") as f:
        return json.load(f)["files"]


class ReadyTraceWorld(tc.TraceWorld):
    """TraceWorld with the Vote the start state does not restate."""

    def __init__(self, p):
        super().__init__(p)
        if p.trace in VOTED_FOR_1:
            for n in self.nodes:
                n.vote = 0


def world_state(w):
    """The World's rows as qe_progress and qe_follower name them."""
    st = osim.world_state(w)
    ns = w.nodes
    st.term, st.state = [n.term for n in ns], [n.state for n in ns]
    st.lead, st.vote = [n.lead for n in ns], [n.vote for n in ns]
    return st


def fresh_rows(G):
    u64, u8 = np.uint64, np.uint8
    return rdm.ready_state(stable=np.zeros(G, u64), applied=np.zeros(G, u64),
                           snap_pending=np.zeros(G, u64), prev_term=np.zeros(G, u64),
                           prev_commit=np.zeros(G, u64), prev_vote=np.zeros(G, u8),
                           prev_lead=np.zeros(G, u8), prev_state=np.zeros(G, u8))


def start_rows(be):
    """NewRawNode on the World, applied = committed, and KNEW_A_LEADER."""
    p, w = be.p, be.w
    rs = fresh_rows(p.G)
    rdm.reset(world_state(w), rs)
    rs.applied[:] = [n.committed for n in w.nodes]
    for node in KNEW_A_LEADER.get(getattr(p, "trace", None), ()):
        for g in range(p.G):
            if (g - p.gbase) % p.N + 1 == node:
                rs.prev_lead[g] = (node % p.N)  # a slot other than None (and not its own)
    return rs


class ReadyRows:
    """A mixin over a cluster_sim backend: the rows of qe_ready_state beside
    the World (`self.rs`, set by the subclass), the note inside the follower /
    snapshot calls, and the two list calls on tests/ready_model.py.  Negative
    controls: note=False leaves the note calls out, move_stable=False makes
    the advance leave `stable` alone, sync_from_commit=True computes MustSync
    from the whole HardState."""

    note, move_stable, sync_from_commit = True, True, False

    def follow(self, msgs):
        outs = super().follow(msgs)
        if self.note:
            rdm.note(world_state(self.w), self.rs,
                     follow_result=[o["result"] for o in outs],
                     append_from=[o.get("append_from", 0) for o in outs])
        return outs

    def snap(self, msgs):
        outs = super().snap(msgs)
        if self.note:
            rdm.note(world_state(self.w), self.rs, snap_result=[o["result"] for o in outs],
                     snap_resp_index=[o.get("resp_index", 0) for o in outs])
        return outs

    def list_ready(self, pending=None):
        recs, _ = rdm.ready(world_state(self.w), self.rs, pending=pending, ent_runs=cs.MSG_RUNS,
                            sync_from_commit=self.sync_from_commit)
        return recs

    def advance_ready(self, recs):
        return rdm.advance(world_state(self.w), self.rs, recs, move_stable=self.move_stable)


class ReadyModelBackend(ReadyRows, tc.TraceModelBackend):
    WORLD = ReadyTraceWorld

    def __init__(self, p, note=True, move_stable=True, sync_from_commit=False, **kw):
        super().__init__(p, **kw)
        self.note, self.move_stable, self.sync_from_commit = note, move_stable, sync_from_commit
        self.rs = start_rows(self)


def describe(rec):
    """A record in the terms of a printed Ready."""
    if rec is None:
        return dict(must_sync=False, soft=None, hard=None, entries=[], committed=[], snapshot=None)
    f = rec["flags"]
    lead = 0 if rec["lead"] == rdm.NONE else rec["lead"] + 1
    vote = 0 if rec["vote"] == rdm.NONE else rec["vote"] + 1
    return dict(
        must_sync=bool(f & rdm.MUST_SYNC),
        soft=f"Lead:{lead} State:{tc.STATE_NAME[rec['state']]}" if f & rdm.SOFT else None,
        hard=[rec["term"], vote, rec["commit"]] if f & rdm.HARD else None,
        entries=rdm.expand(rec["ent_first"], rec["ents"]),
        committed=rdm.expand(rec["apply_first"], rec["apply"]),
        snapshot=rec["snap_index"] if f & rdm.SNAP else None)


class ReadyReplay(tc.Replay):
    def __init__(self, name, tr, be, blocks):
        super().__init__(name, tr, be)
        self.gold = [b for b in blocks[name] if b["cmd_line"] >= be.p.start]
        self.compared = 0

    def ready(self, node, block):
        p, be = self.p, self.be
        self.expect(self.compared < len(self.gold), "a Ready block the golden file does not hold")
        gold = self.gold[self.compared]
        self.expect((gold["cmd_line"], gold["node"]) == (self.line, node),
                    f"the golden block is {gold['cmd_line']} / node {gold['node']}")
        pending = np.zeros(p.G, np.uint8)
        pending[self.group(node)] = bool(self.pending[node])  # its messages: the lists' half
        mine = [r for r in be.list_ready(pending) if r["group"] == p.goff + self.group(node)]
        self.expect(len(mine) <= 1, "a group listed twice")
        rec = mine[0] if mine else None
        self.expect(rec is not None or not self.pending[node], "pending set, no record")
        if rec is not None:
            self.expect(not rec["flags"] & (rdm.ENTS_CUT | rdm.APPLY_CUT), f"a cut list: {rec}")
        got = describe(rec)
        want = {k: gold[k] for k in got}
        self.expect(got == want, f"Ready at file line {gold['line']}: record {got}, "
                                 f"the reference printed {want}")
        self.compared += 1
        if rec is not None:
            res = be.advance_ready([rec])
            self.expect(list(res) == [rdm.ADV_OK], f"qe_advance: {list(res)}")
        super().ready(node, block)

    def finish(self):
        super().finish()
        self.expect(self.compared == len(self.gold) == BLOCKS.get(self.name, len(self.gold)),
                    f"{self.compared} of {len(self.gold)} Ready blocks compared")


def replay(name, blocks=None, **kw):
    """One trace on the model backend -> the ReadyReplay (its counters)."""
    tr = traces()[name]
    be = ReadyModelBackend(tc.params(name, tr), **kw)
    return ReadyReplay(name, tr, be, blocks or ready_blocks()).run()


# ---------------------------------------------------------------------------
# The closed loop on tests/cluster_sim.py: a Storage per node rebuilt from the
# records alone
# ---------------------------------------------------------------------------
class ClusterReadyModel(ReadyRows, cs.ModelBackend):
    def __init__(self, p, **kw):
        super().__init__(p, **kw)
        self.rs = start_rows(self)


class StorageMismatch(AssertionError):
    pass


class ReadySim(cs.Sim):
    """Sim with `ready` + `advance` at the end of every round, and before
    every compaction (a host compacts what it has applied).  Per node a Storage
    is kept from the records alone: the HardState, the entries written at
    ent_first truncating what lies above, the snapshot; and the apply cursor."""

    def __init__(self, p, backend, **kw):
        super().__init__(p, backend, **kw)
        ns = self.w.nodes
        self.hard = [(n.term, n.vote, n.committed) for n in ns]
        self.log = [dict(n.ents) for n in ns]           # index -> term
        self.snap = [n.ents[0][0] for n in ns]          # the newest snapshot stored
        self.applied = [n.committed for n in ns]
        self.seen = Counter()

    def check(self, ok, what):
        if not ok:
            raise StorageMismatch(f"round {self.round_no}: {what}")

    def store(self, r):
        p = self.p
        g = r["group"] - p.goff
        f = r["flags"]
        self.seen["records"] += 1
        if f & rdm.SNAP:
            i = r["snap_index"]
            self.log[g] = {k: t for k, t in self.log[g].items() if k > i}
            self.snap[g], self.applied[g] = i, i
            self.seen["snapshots"] += 1
        if r["ent_count"]:
            first = r["ent_first"]
            self.check(sum(n for n, _ in r["ents"]) == r["ent_count"], f"run rows of {r}")
            self.seen["truncations"] += any(k >= first for k in self.log[g])
            self.log[g] = {k: t for k, t in self.log[g].items() if k < first}
            for t, i in rdm.expand(first, r["ents"]):
                self.log[g][i] = t
            self.seen["entries"] += r["ent_count"]
            self.seen["ents_cut"] += bool(f & rdm.ENTS_CUT)
        if f & rdm.HARD:
            self.hard[g] = (r["term"], r["vote"], r["commit"])
            self.seen["hard"] += 1
        self.check(bool(f & rdm.MUST_SYNC) >= bool(r["ent_count"]), f"MustSync of {r}")
        if r["apply_count"]:
            self.check(r["apply_first"] == self.applied[g] + 1,
                       f"group {g}: applies from {r['apply_first']} after {self.applied[g]}")
            self.applied[g] = r["apply_first"] + r["apply_count"] - 1
            self.seen["applied"] += r["apply_count"]
        self.check(self.applied[g] <= r["commit"], f"group {g}: applied past committed: {r}")

    def drain(self):
        while True:
            recs = self.be.list_ready()
            self.check(len({r["group"] for r in recs}) == len(recs), "a group listed twice")
            for r in recs:
                self.store(r)
            res = self.be.advance_ready(recs)
            self.check(all(x == rdm.ADV_OK for x in res), f"qe_advance: {sorted(set(res))}")
            if not any(r["flags"] & (rdm.ENTS_CUT | rdm.APPLY_CUT) for r in recs):
                return

    def do_compact(self, at):
        self.drain()
        super().do_compact(at)

    def round(self):
        view = super().round()
        self.drain()
        return view

    def run(self):
        super().run()
        self.check(self.be.list_ready() == [], "a Ready left after the last advance")
        for g, (hard, n) in enumerate(zip(*self.resident())):
            self.check(self.hard[g] == hard, f"group {g}: stored HardState {self.hard[g]}, "
                                             f"resident {hard}")
            dummy = n[0][0]
            mine = sorted((i, t) for i, t in self.log[g].items() if i > dummy)
            self.check(mine == n[1:], f"group {g}: stored log {mine[-6:]}, resident {n[-6:]}")
            self.check(self.applied[g] == hard[2], f"group {g}: applied {self.applied[g]}")
        return self

    def resident(self):
        """-> per group the resident HardState and the resident log [(index,
        term), ...] from the dummy entry on.  Here: the models' (a device
        backend reads its rows back)."""
        ns = self.w.nodes
        hard = [(n.term, n.vote if n.vote < self.p.N else rdm.NONE, n.committed) for n in ns]
        return hard, [list(n.ents) for n in ns]
