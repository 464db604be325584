"""The reference's interaction traces replayed with ALL roles on one resident
state, every message a node steps on built by another node's outbox / replies
records (tests/golden/interaction_traces.json: what the reference printed).

One trace is one cluster: node i is group base + i - 1, sits in slot i - 1 and
has self_slot = i - 1 (the layout of tests/cluster_sim.py); every group carries
every row family at once (cluster_sim.World's rows).  Every other group of the
batch holds a copy of the initial state of the node whose slot it falls on and
takes no message.  Membership follows the trace: a node created later by
`add-nodes` exists from the start as an empty group (term 0, dummy entry (0, 0),
no configuration); the host's conf-change application between Readies (the new
masks; switchToConfig through qe_switch_config on a leader) is written out in
HOOKS where the trace prints "switched to configuration".

The driver (`Replay`) walks the fixture's commands and blocks in file order
against a backend with one method per entry point (`TraceModelBackend` here:
the follower, vote, snapshot and tick models, the C oracle for the leader half,
outbox_model / replies_model / inbox_model for the lists;
tests/test_gpu_trace_cluster.py runs the engine beside it).  It keeps ONE pool
of in-flight records, FIFO per (from, to, type).  Every record in the pool came
out of qe_outbox or qe_replies (or their models): no message is ever built from
the fixture's fields.

  campaign n         a HUP record through qe_inbox into qe_vote_step; a won
                     election's `elected` row goes to qe_become_leader (BCAST)
  propose n          qe_propose at n (propose-conf-change: a conf-change entry)
  tick-heartbeat n   one qe_tick; hb_sent / hb_commit through qe_outbox
  recv block of X    the block's messages are taken out of the pool (the oldest
                     of that (from, to, type); one the pool does not hold is a
                     failure), handed to qe_inbox as one list, the step calls
                     run on the rows it routes, the deferred list is fed back
                     until it is empty; qe_outbox after every leader-side call,
                     qe_replies after every receiver-side call; the records are
                     X's pending output
  ready block of X   X's pending records, in order per destination, must equal
                     the block's messages in every field the fixture holds for
                     the type: type, to, term; index, logterm, commit; reject
                     and hint; entries as the (term, index) list the record's
                     term runs expand to; snap_index for MsgSnap.  HardState
                     (term, commit), lead_state and the entries list (appended
                     since the last Ready, then newly committed) where printed.
  status block       every Progress through trace_replay.progress_string
  debug lines        "decreased progress of X to [...]", "cast" / "rejected
                     MsgVote", "has received G ... votes and R vote rejections"

At the end the pool must hold exactly what the fixture lists as sent and never
as received, and the per-type counts of sent and received messages must be
COUNTS (computed from the fixture: 106 sent records in the five traces).

What the fixture cannot witness, and is therefore not compared: a MsgSnap's
snapshot term and ConfState (the fixture holds snap_index alone), a heartbeat's
context, and the Commit a MsgVote carries (the reference sets none).

Traces that run (all five mandatory ones, every message compared):
campaign.txt (run table of ONE row: every node sits on a snapshot of the term
the first leader wins, so becomeLeader enters the last run and appends none),
campaign_learner_must_vote.txt, probe_and_replicate.txt,
snapshot_succeed_via_app_resp.txt, confchange_v1_remove_leader.txt.
Beside them confchange_v1_add_single.txt and confchange_v2_add_single_auto.txt
(a voter joins a one-node cluster and is caught up by snapshot), from the state
trace_replay.LEADER_START restates: after the first Ready of `stabilize` applied
the conf change, with switchToConfig (qe_switch_config) as the first call.
Left out: confchange_v2_add_double_implicit.txt, confchange_v2_add_single_
explicit.txt and confchange_v2_add_double_auto.txt.  They pass through joint
configurations, which need the outgoing-voters mask (`out`) that
cluster_sim.World and the device backend built on it do not carry, and the
leader's apply-time auto-leave append (QE_PROP_APPEND_ONLY), which the backend
has no method for; tests/trace_replay.py replays them from the leader's side.
None of them is half compared here.

ALLOWED lists the deviations that are the engine's documented contract: only
H7's coalescing of several sends to one peer within one call (the record then
equals the reference's first message in Index and LogTerm and carries the
concatenation of their entries).  It is EMPTY: no call of the five traces sends
twice to one peer.  An entry is checked for exactly that relaxed form, never
skipped.

R per trace (RUNS) is the largest number of term runs any node of the trace
holds at any point, computed from the fixture (run_capacity) and asserted; the
replay also asserts that the table was filled to the last row.  No slack.
This module imports no torch.
"""
import copy
import re
from collections import Counter

import numpy as np

from oracle import orc
from tests import cluster_sim as cs
from tests import follower_model as fm
from tests import inbox_model as im
from tests import outbox_model as om
from tests import outbox_sim as osim
from tests import replies_sim as rsim
from tests import snapshot_model as sm
from tests import tick_model as tm
from tests import vote_model as vm
from tests.follower_traces import INITIAL
from tests.progress_scenarios import PF_PROBE_SENT, PF_RECENT_ACTIVE, peer_view
from tests.trace_replay import (LEADER_START, SW_PROBE, SW_REMOVED, command, parse_progress,
                                progress_string, traces)
from tests.vote_traces import CANDIDATES, VOTERS

MANDATORY = ("campaign.txt", "campaign_learner_must_vote.txt", "probe_and_replicate.txt",
             "snapshot_succeed_via_app_resp.txt", "confchange_v1_remove_leader.txt")
OPTIONAL = ("confchange_v1_add_single.txt", "confchange_v2_add_single_auto.txt")
TRACES = MANDATORY + OPTIONAL
# (trace, command line, reason): H7 coalescings.  None occurs.
ALLOWED = []
# the run-table capacity of each trace (run_capacity computes it from the fixture)
RUNS = {"campaign.txt": 1, "campaign_learner_must_vote.txt": 2, "probe_and_replicate.txt": 5,
        "snapshot_succeed_via_app_resp.txt": 1, "confchange_v1_remove_leader.txt": 1,
        "confchange_v1_add_single.txt": 1, "confchange_v2_add_single_auto.txt": 1}
# per trace: (sent by type, received by type), counted in the fixture
COUNTS = {
    "probe_and_replicate.txt": ({"MsgVote": 6, "MsgVoteResp": 6, "MsgApp": 19, "MsgAppResp": 17},
                                {"MsgVote": 6, "MsgVoteResp": 6, "MsgApp": 17, "MsgAppResp": 17}),
    "snapshot_succeed_via_app_resp.txt": (
        {"MsgHeartbeat": 2, "MsgHeartbeatResp": 2, "MsgSnap": 1, "MsgAppResp": 2, "MsgApp": 1},
        {"MsgHeartbeat": 2, "MsgHeartbeatResp": 2, "MsgSnap": 1, "MsgAppResp": 2, "MsgApp": 1}),
    "campaign.txt": ({"MsgVote": 2, "MsgVoteResp": 2, "MsgApp": 4, "MsgAppResp": 4},
                     {"MsgVote": 2, "MsgVoteResp": 2, "MsgApp": 4, "MsgAppResp": 4}),
    "campaign_learner_must_vote.txt": (
        {"MsgVote": 2, "MsgVoteResp": 1, "MsgApp": 4, "MsgAppResp": 3},
        {"MsgVote": 1, "MsgVoteResp": 1, "MsgApp": 3, "MsgAppResp": 3}),
    "confchange_v1_remove_leader.txt": (
        {"MsgApp": 12, "MsgAppResp": 12, "MsgHeartbeat": 2, "MsgHeartbeatResp": 2},
        {"MsgApp": 12, "MsgAppResp": 12, "MsgHeartbeat": 2, "MsgHeartbeatResp": 2}),
}
for _name in OPTIONAL:
    COUNTS[_name] = ({"MsgApp": 2, "MsgAppResp": 3, "MsgSnap": 1},
                     {"MsgApp": 2, "MsgAppResp": 3, "MsgSnap": 1})
SENT_TOTAL = 106  # in the mandatory set
assert sum(sum(COUNTS[n][0].values()) for n in MANDATORY) == SENT_TOTAL
# nodes that take no step in the printed part and that neither INITIAL nor
# CANDIDATES restates: node 1 of campaign_learner_must_vote.txt, the deposed
# leader whose messages are dropped (`deliver-msgs drop`); its log is the one
# CANDIDATES gives node 2, which followed it.
SILENT = {"campaign_learner_must_vote.txt": {1: ([(3, 1), (4, 1)], 4, 1, None)}}
F_CAP = 8        # Inflights capacity: the 16-bit form's largest; no trace fills it
ET = 10          # election timeout in ticks: no trace ticks that often
TYPE_NAME = {im.APP: "MsgApp", im.SNAP: "MsgSnap", im.HEARTBEAT: "MsgHeartbeat",
             im.APP_RESP: "MsgAppResp", im.APP_RESP_REJECT: "MsgAppResp",
             im.HEARTBEAT_RESP: "MsgHeartbeatResp", im.VOTE: "MsgVote",
             im.VOTE_RESP: "MsgVoteResp"}
STATE_NAME = {fm.ST_FOLLOWER: "StateFollower", vm.ST_CANDIDATE: "StateCandidate",
              fm.ST_LEADER: "StateLeader", vm.ST_PRE_CANDIDATE: "StatePreCandidate"}


class TraceMismatch(AssertionError):
    """The replay left the trace at command line `line` of `trace`."""

    def __init__(self, trace, line, what):
        super().__init__(f"{trace}:{line}: {what}")
        self.trace, self.line, self.what = trace, line, what


def mask(ids):
    return sum(1 << (i - 1) for i in ids)


# ---------------------------------------------------------------------------
# The initial state of every node, from the restatements the tree holds
# ---------------------------------------------------------------------------
def node_spec(ents, committed, term, lead, voters, learners=(), leader=None):
    return dict(ents=ents, committed=committed, term=term, lead=lead, voters=tuple(voters),
                learners=tuple(learners), leader=leader)


def first_hard_state(cmds, n, start):
    """The commit of node n's first HardState line at or after `start`."""
    for c in cmds:
        if c["line"] < start:
            continue
        for b in c["blocks"]:
            node = b.get("node") if b.get("node") is not None else int(c["cmd"].split()[1])
            if b["kind"] == "ready" and node == n and "commit" in b:
                return b["commit"]
    raise AssertionError(f"no HardState of node {n}")


def reported_term(cmds, n, start, default):
    """The term the trace reports node n at before its first message ("INFO n
    [term: T] received ...")."""
    for c in cmds:
        if c["line"] < start:
            continue
        for b in c["blocks"]:
            for d in b.get("debug", []):
                t = re.match(rf"INFO {n} \[term: (\d+)\] received", d)
                if t:
                    return int(t.group(1))
    return default


def setup(name, tr):
    """-> (S, the first command line replayed, {node id: node_spec})."""
    cmds = tr["commands"]
    add = [c for c in cmds if c["cmd"].startswith("add-nodes")]
    m = re.match(r"add-nodes (\d+)(?: voters=\(([\d,]+)\))?(?: learners=\(([\d,]+)\))?"
                 r"(?: index=(\d+))?", add[0]["cmd"])
    snap = int(m.group(4))
    voters0 = tuple(int(x) for x in m.group(2).split(","))
    learners0 = tuple(int(x) for x in m.group(3).split(",")) if m.group(3) else ()
    S = sum(int(re.match(r"add-nodes (\d+)", c["cmd"]).group(1)) for c in add)
    dumps = {int(c["cmd"].split()[1]): [(i, t) for t, i in c["log"]]
             for c in cmds if c["cmd"].startswith("raft-log ")}
    nodes = {}

    def log_of(n, log):
        return [(snap, 1)] + (dumps[n] if log == "raft-log" else list(log))

    if name in CANDIDATES:
        cand, clog, cterm, clead, cvoters = CANDIDATES[name]
        start = [c for c in cmds if c["cmd"] == f"campaign {cand}"][-1]["line"]
        assert VOTERS[name] == voters0
        for n in range(1, S + 1):
            if n == cand:
                log, commit, term, lead, voters = clog, None, cterm, clead, cvoters
            else:
                log, commit, term, lead = INITIAL[name].get(n) or SILENT[name][n]
                voters = voters0 if n in INITIAL[name] else cvoters
                term = reported_term(cmds, n, start, term)
            ents = log_of(n, log)
            if commit is None:
                commit = first_hard_state(cmds, n, start)
            learners = tuple(x for x in learners0 if x not in voters)
            nodes[n] = node_spec(ents, commit, term, lead, voters, learners)
    else:
        ls = LEADER_START[name]
        start = command(cmds, ls["start"])["line"]
        peers = ls.get("peers")
        if peers is None:  # the Progress the trace's `status 1` prints there
            st = command(cmds, ls["start"])["blocks"][0]["progress"]
            peers = [parse_progress(st[str(k)]) for k in range(1, S + 1)]
        dummy = ls["runs"][0]
        ents = [(dummy[0], dummy[1])] + [(i, ls["term"])
                                         for i in range(dummy[0] + 1, ls["last_index"] + 1)]
        voters1 = ls.get("voters", voters0)  # (a conf change applied before the start)
        nodes[1] = node_spec(ents, ls["committed"], ls["term"], 1, voters1, leader=dict(
            peers=peers, pci=ls["pci"], snap_index=ls["snap_index"], term_start=ls["term_start"]))
        for n in range(2, S + 1):
            if n in INITIAL.get(name, {}):
                log, commit, term, lead = INITIAL[name][n]
                nodes[n] = node_spec(log_of(n, log), commit, term, lead, voters0)
            else:  # created by a later `add-nodes`: empty, no configuration
                nodes[n] = node_spec([(0, 0)], 0, 0, None, ())
    return S, start, nodes


def run_capacity(name, tr):
    """The largest number of term runs any node of the trace holds at any
    point, from the fixture alone: the initial logs, every MsgApp a node sends
    (its own log holds Index and the entries) or receives where its log holds
    (Index, LogTerm), and every MsgSnap received (the log restarts there)."""
    S, start, nodes = setup(name, tr)
    logs = {n: dict(sp["ents"]) for n, sp in nodes.items()}
    dummy = {n: sp["ents"][0][0] for n, sp in nodes.items()}

    def runs(n):
        idx = sorted(i for i in logs[n] if i >= dummy[n])
        return 1 + sum(logs[n][a] != logs[n][b] for a, b in zip(idx, idx[1:]))

    best = max(runs(n) for n in logs)
    for c in tr["commands"]:
        if c["line"] < start:
            continue
        for b in c["blocks"]:
            for m in b.get("msgs", []):
                n = m["from"] if b["kind"] == "ready" else m["to"]
                if m["type"] == "MsgSnap" and b["kind"] == "recv":
                    line = [d for d in b["debug"] if "restored snapshot" in d][0]
                    i, t = map(int, re.search(r"\[index: (\d+), term: (\d+)\]", line).groups())
                    logs[n], dummy[n] = {i: t}, i
                elif m["type"] == "MsgApp" and m["entries"]:
                    if b["kind"] == "recv" and logs[n].get(m["index"]) != m["logterm"]:
                        continue  # rejected
                    for t, i in m["entries"]:
                        if logs[n].get(i) != t:  # a conflict truncates
                            logs[n] = {k: v for k, v in logs[n].items() if k < i}
                        logs[n][i] = t
                best = max(best, runs(n))
    return best


# ---------------------------------------------------------------------------
# The composed model of the batch
# ---------------------------------------------------------------------------
def params(name, tr, G=None, gbase=0, goff=0, ring16=False):
    """cluster_sim.Params for one trace: N = S = the trace's node count, the
    cluster at groups [gbase, gbase + N), G groups in all (default: N)."""
    S, start, nodes = setup(name, tr)
    p = cs.Params(N=S, C=1, R=RUNS[name], F=F_CAP, ring16=ring16, flags=0, goff=goff, ET=ET)
    p.G = G or S
    p.stride = p.G + 3
    p.gbase, p.init, p.start, p.trace = gbase, nodes, start, name
    assert gbase + S <= p.G
    return p


class TraceWorld(cs.World):
    """cluster_sim.World with each group's rows composed from a node_spec; the
    configuration is per group (`confs`, the nodes' inc / tracked and the
    leader half's inc / tracked rows say the same)."""

    def __init__(self, p):
        self.p = p
        G, N, st = p.G, p.N, p.stride
        md = orc.mask_dtype(N)
        self.inc = self.learner = 0  # per group here: see `confs`
        self.nodes, self.confs, self.snap_index = [], [], []
        self.tm = m = tm.Model(G, N, p.ET, 1, False, seed=p.seed, goff=p.goff, stride=st)
        self.pb = pb = orc.ProgressBatch(G, N, p.F, p.R, stride=st, max_ents=0)
        pb.ring16 = bool(p.ring16)
        pb.inc, pb.tracked = np.zeros(G, md), np.zeros(G, md)
        pb.self_slot = np.zeros(G, np.uint8)
        pb.lead_transferee = np.full(G, cs.NONE, np.uint8)
        pb.snap_index = np.zeros(G, np.uint64)
        pb.track_reads()
        self.pci, self.unc = np.zeros(G, np.uint64), np.zeros(G, np.uint64)
        m.peer, m.match, m.committed = pb.pw, pb.match, pb.committed
        m.lead_transferee, m.self_slot = pb.lead_transferee, pb.self_slot
        m.inc, m.tracked = pb.inc, pb.tracked
        m.read_head, m.read_count = pb.read_head, pb.read_count
        m.rt[:] = p.ET + np.arange(G) % p.ET
        for g in range(G):
            nid = (g - p.gbase) % N + 1
            sp = p.init[nid]
            inc, lrn = mask(sp["voters"]), mask(sp["learners"])
            lead = cs.NONE if sp["lead"] is None else sp["lead"] - 1
            n = vm.Node(sp["ents"], committed=sp["committed"], term=sp["term"], lead=lead,
                        state=fm.ST_LEADER if sp["leader"] else fm.ST_FOLLOWER,
                        self_slot=nid - 1, inc=inc, tracked=inc | lrn)
            self.nodes.append(n)
            self.confs.append(sm.Conf(N, inc, 0, lrn, ids=[s + 1 for s in range(N)]))
            pb.inc[g], pb.tracked[g], pb.self_slot[g] = inc, inc | lrn, nid - 1
            ld = sp["leader"]
            self.snap_index.append(ld["snap_index"] if ld else sp["ents"][0][0])
            for s in range(N):
                k = s * st + g
                pb.next[k] = n.last_index() + 1
                if ld:
                    q = ld["peers"][s]
                    pb.match[k], pb.next[k], pb.pending[k] = q["match"], q["next"], q["pending"]
                    pb.pw[k] = orc.pack_word(
                        q["state"] | (PF_PROBE_SENT if q["probe_sent"] else 0) |
                        (PF_RECENT_ACTIVE if q["recent_active"] else 0), 0, 0)
            if ld:
                self.pci[g], pb.term_start[g] = ld["pci"], ld["term_start"]
            self.push(g)

    def set_conf(self, g, inc, learner):
        """The host applied a conf change at group g: the new masks."""
        n = self.nodes[g] = copy.deepcopy(self.nodes[g])
        n.inc, n.tracked = inc, inc | learner
        old = self.confs[g]
        self.confs[g] = sm.Conf(self.p.N, inc, 0, learner, ids=old.ids)
        self.pb.inc[g], self.pb.tracked[g] = inc, inc | learner

    def put_snode(self, g, sn):
        """A restore replaces the configuration: every holder follows."""
        super().put_snode(g, sn)
        c = sn.conf
        n = self.nodes[g]
        if (n.inc, n.tracked) != (c.inc, c.tracked):
            n = self.nodes[g] = copy.deepcopy(n)
            n.inc, n.tracked = c.inc, c.tracked
        self.pb.inc[g], self.pb.tracked[g] = c.inc, c.tracked


class TraceHost:
    """What a trace needs of a backend beyond the simulation's entry points,
    on the models (a mixin over cluster_sim.ModelBackend): a conf-change
    proposal with the applied row, qe_switch_config, qe_inbox, the host's
    mask rewrite."""

    WORLD = TraceWorld

    def init_trace(self):
        self.applied = np.array([n.committed for n in self.w.nodes], np.uint64)

    def cc_rows(self, cc):
        """cc: None or {group: leave_joint} -> orc.propose's arrays (one
        conf-change entry at position 0)."""
        if cc is None:
            return None
        G = self.p.G
        cnt, pos = np.zeros(G, np.uint8), np.zeros(G, np.uint32)
        lv, sz = np.zeros(G, np.uint8), np.zeros(G, np.uint32)
        for g, leave in cc.items():
            cnt[g], lv[g] = 1, int(leave)
        return 1, cnt, pos, lv, sz

    def model_propose(self, num_entries, cc):
        w = self.w
        self.calls["propose"] += 1
        o = orc.propose(w.pb, num_entries, cc=self.cc_rows(cc), applied=self.applied,
                        pending_conf_index=w.pci, uncommitted_size=w.unc, goff=self.p.goff)
        for g in np.flatnonzero(num_entries):
            w.pull(g)
        return o

    def model_switch_config(self, switched):
        w = self.w
        self.calls["switch_config"] += 1
        o = orc.switch_config(w.pb, switched, goff=self.p.goff)
        for g in np.flatnonzero(switched):
            w.pull(g)
        return o

    def model_route(self, recs, tick_action=None):
        w, p = self.w, self.p
        st = im.state(num_groups=p.G, group_offset=p.goff, num_slots=p.N, stride=p.stride,
                      term=[n.term for n in w.nodes], state=[n.state for n in w.nodes])
        return im.route(st, recs, tick_action, cs.MSG_RUNS)

    def set_conf(self, g, inc, learner):
        self.w.set_conf(g, inc, learner)


class TraceModelBackend(TraceHost, rsim.ModelReplies, osim.ModelOutbox):
    """ModelBackend on a TraceWorld whose leader-side calls leave qe_outbox's
    records in `outbox` and whose receiver-side calls leave qe_replies' in
    `replies` (tests/outbox_sim.py, tests/replies_sim.py).
    outbox_fault: a negative control -- "log_term_next": a MsgApp's log_term is
    the term of index + 1; "commit_before": its commit is the one from before
    the call."""

    def __init__(self, p, outbox_fault=None, **kw):
        super().__init__(p, **kw)
        self.outbox_fault = outbox_fault
        self.init_trace()
        self.com0 = self.w.pb.committed.copy()

    # ---- the record lists ----
    def list_records(self, **inp):
        if any(k in inp for k in ("sent", "snap", "hb_sent")):
            return self.list_outbox(**inp)
        return rsim.ModelReplies.list_records(self, **inp)

    def list_outbox(self, **inp):
        w = self.w
        osim.ModelOutbox.list_records(self, **inp)
        st = osim.world_state(w)
        for (g, s), r in self.outbox.items():
            if r["type"] != om.APP:
                continue
            if self.outbox_fault == "log_term_next":
                r["log_term"] = om.term_at(om.runs_of(st, g), int(st.last_index[g]), r["index"] + 1)
            elif self.outbox_fault == "commit_before":
                r["commit"] = int(self.com0[g])

    def take(self):
        """-> (the outbox records, the replies records) of the calls since the
        last take, each in list order."""
        ob, rp = list(self.outbox.values()), list(self.replies.values())
        self.outbox, self.replies = {}, {}
        return ob, rp

    def before_leader_call(self):
        self.com0 = self.w.pb.committed.copy()

    def become_leader(self, elected):
        self.before_leader_call()
        return super().become_leader(elected)

    def progress_step(self, mtype, mindex, mhint, mlogterm):
        self.before_leader_call()
        return super().progress_step(mtype, mindex, mhint, mlogterm)

    def propose(self, num_entries, cc=None):
        self.before_leader_call()
        nxt0 = self.w.pb.next.copy()
        o = self.model_propose(num_entries, cc)
        self.list_records(sent=o.sent, snap=o.snap, next_before=nxt0)
        return o

    def switch_config(self, switched):
        self.before_leader_call()
        nxt0 = self.w.pb.next.copy()
        o = self.model_switch_config(switched)
        self.list_records(sent=o.sent, snap=o.snap, next_before=nxt0)
        return o

    def route(self, recs, tick_action=None, carry=0):
        return self.model_route(recs, tick_action)


# ---------------------------------------------------------------------------
# The host's conf-change application between Readies
# ---------------------------------------------------------------------------
def hook_remove_leader(rp, node, block):
    if any(x.endswith("switched to configuration voters=(2 3)") for x in block["debug"]):
        g = rp.group(node)
        rp.be.set_conf(g, 0b110, 0)
        if rp.be.w.nodes[g].state == fm.ST_LEADER:
            # the removed leader returns at once (raft.go:1663-1674)
            sw = np.zeros(rp.p.G, np.uint8)
            sw[g] = 1
            o = rp.be.switch_config(sw)
            rp.expect(int(o.result[g]) == SW_REMOVED, f"switchToConfig: {o.result[g]}")
            rp.collect(node)
        rp.switched += 1


def hook_learner(rp, node, block):
    if any(x.endswith("switched to configuration voters=(1 2 3)") for x in block["debug"]):
        rp.be.set_conf(rp.group(node), 0b111, 0)
        rp.switched += 1


HOOKS = {"confchange_v1_remove_leader.txt": (hook_remove_leader, 3),
         "campaign_learner_must_vote.txt": (hook_learner, 1)}


# ---------------------------------------------------------------------------
# The driver
# ---------------------------------------------------------------------------
def expand(rec):
    """The (term, index) list a MsgApp record's term runs stand for."""
    out, i = [], rec["index"]
    for n, t in rec["ents"]:
        for _ in range(n):
            i += 1
            out.append([t, i])
    return out


def fields(rec):
    """A record in the fixture's terms: what is compared for its type."""
    t = rec["type"]
    d = {"type": TYPE_NAME.get(t, f"type {t}"), "term": rec["term"]}
    if t == im.APP:
        d.update(index=rec["index"], logterm=rec["log_term"], commit=rec["commit"],
                 entries=expand(rec), reject=False, hint=0)
    elif t == im.SNAP:
        d.update(snap_index=rec["index"])
    elif t == im.HEARTBEAT:
        d.update(index=0, logterm=0, commit=rec["commit"], entries=[], reject=False, hint=0)
    elif t in (im.APP_RESP, im.APP_RESP_REJECT):
        d.update(index=rec["index"], logterm=rec["log_term"], commit=0, entries=[],
                 reject=t == im.APP_RESP_REJECT, hint=rec["hint"])
    elif t == im.HEARTBEAT_RESP:
        d.update(index=0, logterm=0, commit=0, entries=[], reject=False, hint=0)
    elif t == im.VOTE:
        d.update(index=rec["index"], logterm=rec["log_term"], entries=[], reject=False, hint=0)
    elif t == im.VOTE_RESP:
        d.update(index=0, logterm=0, commit=0, entries=[],
                 reject=bool(rec["flags"] & vm.VMF_REJECT), hint=0)
    return d


def wanted(m, keys):
    return {k: m[k] for k in keys}


class Replay:
    def __init__(self, name, tr, be):
        self.name, self.cmds, self.be, self.p = name, tr["commands"], be, be.p
        p = self.p
        self.pool = []                                   # in-flight records, in sending order
        self.pending = {n: [] for n in range(1, p.N + 1)}  # a node's records since its last Ready
        self.unstable = {n: None for n in self.pending}  # first index appended since then
        self.line = 0
        self.sent, self.received, self.checked = Counter(), Counter(), Counter()
        self.switched = 0
        self.max_runs = max(len(n.runs) for n in be.w.nodes)
        self.owed_tallies = []

    # ---- helpers ----
    def group(self, node):
        return self.p.gbase + node - 1

    def node(self, node):
        return self.be.w.nodes[self.group(node)]

    def fail(self, what):
        raise TraceMismatch(self.name, self.line, what)

    def expect(self, ok, what):
        if not ok:
            self.fail(what)

    def collect(self, node, counts=None):
        """The records of the calls just made -> node's pending output, as
        in-flight records (the receiver's group, the sender's slot)."""
        p = self.p
        ob, rp = self.be.take()
        me = p.goff + self.group(node)
        for r in ob + rp:
            if r["group"] != me:
                # a copy's record (a tick reaches every group): never sent
                self.expect(not p.gbase <= r["group"] - p.goff < p.gbase + p.N,
                            f"a record of another node of the cluster: {r}")
                continue
            self.expect(r["type"] != om.BAD, f"a BAD record: {r}")
            q = im.rec(p.goff + p.gbase + r["to"], node - 1, r["type"], r["term"], r["index"],
                       r["log_term"], r.get("commit", 0), r.get("hint", 0), r.get("ctx", 0),
                       r.get("flags", 0), r.get("ents", ()))
            q["to_node"], q["from_node"] = r["to"] + 1, node
            q["count"] = (counts or {}).get(r["to"], 1) if r["type"] == im.APP else 1
            self.pending[node].append(q)
        self.max_runs = max(self.max_runs, max(len(n.runs) for n in self.be.w.nodes))

    def settle(self, outs):
        ev = np.array([o["events"] for o in outs], np.uint8)
        if ev.any():
            self.be.tick(ev, 0)
            self.be.take()

    def appended(self, node, first):
        u = self.unstable[node]
        self.unstable[node] = first if u is None else min(u, first)

    # ---- the step calls on the rows qe_inbox routed ----
    def deliver(self, node, recs, tick_action=None, debug=()):
        be, p, w = self.be, self.p, self.be.w
        g = self.group(node)
        queue, carry = recs, 0
        while queue or tick_action is not None:
            out = be.route(queue, tick_action, carry)
            tick_action = None
            for i, d in enumerate(out.disposition):
                self.expect(d in (im.ROUTED, im.DEFERRED),
                            f"disposition {im.ID_NAMES.get(d, d)} of {queue[i]}")
            self.expect(set(out.f) | set(out.s) | set(out.v) | {k[1] for k in out.r} <= {g},
                        "a row of another group")
            if out.f:
                last = w.nodes[g].last_index()
                msgs = [fmsg(out.f.get(x)) for x in range(p.G)]
                outs = be.follow(msgs)
                r = outs[g]["result"]
                self.expect(fm.FR_NONE < r < fm.FR_REFUSED and r != fm.FR_RUNS_FULL,
                            f"qe_follower_step: {fm.FR_NAMES.get(r, r)}")
                if r == fm.FR_APP_ACCEPT and outs[g].get("append_from", 0):
                    self.appended(node, outs[g]["append_from"])
                    assert outs[g]["append_from"] <= last + 1
                self.collect(node)
                self.settle(outs)
            if out.s:
                src = queue[out.s[g]["src"]]
                msgs = [self.smsg(out.s.get(x), src) for x in range(p.G)]
                outs = be.snap(msgs)
                r = outs[g]["result"]
                self.expect(sm.SR_NONE < r < sm.SR_REFUSED, f"qe_snapshot_step: {r}")
                if r == sm.SR_RESTORED:
                    self.unstable[node] = None
                    be.applied[g] = w.nodes[g].committed
                self.collect(node)
                self.settle(outs)
            if out.r:
                n_ = p.N * p.stride
                mt, mi = np.zeros(n_, np.uint8), np.zeros(n_, np.uint64)
                mh, ml = np.zeros(n_, np.uint64), np.zeros(n_, np.uint64)
                for (s, x), r in out.r.items():
                    k = s * p.stride + x
                    mt[k], mi[k], mh[k], ml[k] = r["type"], r["index"], r["hint"], r["log_term"]
                o = be.progress_step(mt, mi, mh, ml)
                counts = {s: int(o.msg_count[s * p.stride + g]) for s in range(p.N)}
                self.collect(node, counts)
            if out.v:
                msgs = [vmsg(out.v.get(x)) for x in range(p.G)]
                was = w.nodes[g].state
                outs = be.vote(msgs)
                o = outs[g]
                self.expect(vm.VR_NONE < o["result"] < vm.VR_REFUSED,
                            f"qe_vote_step: {vm.VR_NAMES.get(o['result'])}")
                self.vote_debug(node, msgs[g], o, was, debug)
                self.collect(node)
                self.settle(outs)
                if o["elected"]:
                    el = np.array([x["elected"] for x in outs], np.uint8)
                    last = w.nodes[g].last_index()
                    bl = be.become_leader(el)
                    self.expect(int(bl.result[g]) == cs.BL_LEADER,
                                f"qe_become_leader refused: result {int(bl.result[g])} "
                                f"(3 = QE_BL_RUNS_FULL) with a run table of {p.R}")
                    self.appended(node, last + 1)
                    self.collect(node)
            carry = len(out.deferred)
            queue = [queue[i] for i in out.deferred]

    def smsg(self, row, src):
        """The ConfState is not in a record: the host's (the sender's
        configuration, which is the snapshot's in every trace here)."""
        if row is None:
            return sm.SMsg()
        c = self.be.w.confs[self.group(src["from_node"])]
        return sm.SMsg(row["type"], row["frm"], row["term"], row["snap_index"], row["snap_term"],
                       c.inc, c.out, c.learner, c.learners_next, c.auto_leave, c.ids)

    def vote_debug(self, node, m, o, was, debug):
        """The trace's "cast" / "rejected" line of a MsgVote and its tally
        lines of a MsgVoteResp."""
        n = self.node(node)
        if m.type == vm.VMSG_VOTE:
            line = [d for d in debug if "cast MsgVote" in d or "rejected MsgVote" in d]
            self.expect(len(line) == 1, "no cast / rejected line")
            self.expect(("cast MsgVote" in line[0]) == (o["result"] == vm.VR_GRANT),
                        f"{line[0]!r} but result {vm.VR_NAMES[o['result']]}")
            lt, li = map(int, re.search(r"\[logterm: (\d+), index: (\d+), vote", line[0]).groups())
            self.expect((lt, li) == (n.last_term(), n.last_index()), line[0])
            self.checked["cast"] += 1
        elif m.type == vm.VMSG_VOTE_RESP and was == vm.ST_CANDIDATE:
            if not self.owed_tallies:
                self.owed_tallies = [tuple(map(int, re.search(
                    r"received (\d+) MsgVoteResp votes and (\d+) vote", d).groups()))
                    for d in debug if "has received" in d]
            self.expect(bool(self.owed_tallies), "no tally line")
            gr, rj = self.owed_tallies.pop(0)
            if o["result"] == vm.VR_PENDING:
                self.expect((gr, rj) == (bin(n.granted).count("1"),
                                         bin(n.voted & ~n.granted).count("1")), "tally")
            else:
                self.expect(o["result"] == vm.VR_WON, f"tally {gr}/{rj}: {o['result']}")
                self.expect(any(f"{node} became leader at term {n.term}" in d for d in debug),
                            "no became-leader line")
            self.checked["tally"] += 1

    # ---- the commands ----
    def campaign(self, node):
        p = self.p
        hup = im.rec(p.goff + self.group(node), node - 1, im.HUP)
        self.deliver(node, [hup])

    def propose(self, c):
        p, be = self.p, self.be
        node = int(c["cmd"].split()[1])
        g = self.group(node)
        ne = np.zeros(p.G, np.uint32)
        ne[g] = 1
        cc = {g: not c["input"]} if c["cmd"].startswith("propose-conf-change") else None
        last = be.w.nodes[g].last_index()
        o = be.propose(ne, cc)
        if c.get("dropped"):
            self.expect(int(o.result[g]) in (2, 3, 4), f"not dropped: {o.result[g]}")
        else:
            self.expect(int(o.result[g]) == 1, f"qe_propose: {o.result[g]}")
            self.expect(int(o.cc_refused[g]) == int(bool(c.get("ignored_cc"))), "cc_refused")
            self.appended(node, last + 1)
        self.collect(node)
        self.checked["proposals"] += 1

    def switch_first(self):
        """The host's work after the Ready the replay starts behind: the conf
        change is applied (the masks are the initial state's), switchToConfig
        finds nothing to commit and probes every peer (raft.go:1682-1692)."""
        g = self.group(1)
        sw = np.zeros(self.p.G, np.uint8)
        sw[g] = 1
        o = self.be.switch_config(sw)
        self.expect(int(o.result[g]) == SW_PROBE, f"switchToConfig: {o.result[g]}")
        self.collect(1)
        self.switched += 1

    def tick_heartbeat(self, node):
        self.be.tick(None, 1)
        self.collect(node)

    # ---- the blocks ----
    def recv(self, node, block):
        recs = []
        for m in block["msgs"]:
            self.expect(m["to"] == node, f"a message to {m['to']} in the block of {node}")
            k = next((i for i, r in enumerate(self.pool)
                      if (r["from_node"], r["to_node"], TYPE_NAME[r["type"]]) ==
                      (m["from"], m["to"], m["type"])), None)
            self.expect(k is not None, f"the pool holds no {m['type']} {m['from']}->{m['to']}")
            r = self.pool.pop(k)
            f = fields(r)
            self.expect(f == wanted(m, f), f"received {wanted(m, f)}, the pool's oldest is {f}")
            self.received[m["type"]] += 1
            recs.append(r)
        self.deliver(node, recs, debug=block["debug"])
        self.expect(not self.owed_tallies, "tally lines left")
        last = {}
        for line in block["debug"]:
            # (the Progress after the round's last change: MaybeDecrTo's line,
            # unless the sendAppend after it turned the peer to StateSnapshot)
            d = (re.search(r"decreased progress of (\d+) to \[(.*)\]", line) or
                 re.search(r"paused sending replication messages to (\d+) \[(.*)\]", line))
            if d:
                last[int(d.group(1))] = d.group(2)
        for peer, text in last.items():
            want, got = parse_progress(text), self.peer(node, peer)
            self.expect(all(got[k] == want[k] for k in ("state", "match", "next", "pending")),
                        f"decreased progress of {peer}: {got}, the trace {text}")
            self.checked["decreased"] += 1

    def peer(self, node, peer):
        pb, st, g = self.be.w.pb, self.p.stride, self.group(node)
        rows = [a.reshape(self.p.N, st)[:, g] for a in (pb.match, pb.next, pb.pending, pb.flags,
                                                       pb.icount)]
        return peer_view(*rows, peer - 1)

    def ready(self, node, block):
        got, want = self.pending[node], [m for m in block["msgs"]]
        self.pending[node] = []
        self.expect(all(m["from"] == node for m in want), "a message of another node")
        for to in sorted({m["to"] for m in want} | {r["to_node"] for r in got}):
            gs = [r for r in got if r["to_node"] == to]
            ws = [m for m in want if m["to"] == to]
            for r in gs:
                f = fields(r)
                n = r["count"]
                self.expect(len(ws) >= n, f"to {to}: a record the trace has no message for: {f}")
                ms, ws = ws[:n], ws[n:]
                if n > 1:  # H7: several sends of one call to one peer, coalesced
                    self.expect(any(a[:2] == (self.name, self.line) for a in ALLOWED),
                                f"to {to}: {n} sends coalesced, not in ALLOWED")
                    w1 = dict(wanted(ms[0], f), entries=[e for m in ms for e in m["entries"]],
                              commit=f["commit"])
                    self.expect(all(m["type"] == "MsgApp" for m in ms) and f == w1,
                                f"to {to}: coalesced {f}, the trace {ms}")
                    self.checked["coalesced"] += 1
                else:
                    self.expect(f == wanted(ms[0], f), f"to {to}: record {f}, the trace "
                                                       f"{wanted(ms[0], f)}")
                self.checked["records"] += 1
            self.expect(not ws, f"to {to}: the trace sends {len(ws)} more: {ws}")
        for m in want:
            self.sent[m["type"]] += 1
        self.pool += got
        # ---- HardState, SoftState, Entries + CommittedEntries ----
        n, g = self.node(node), self.group(node)
        if "term" in block:
            self.expect(block["term"] == n.term, f"HardState term {n.term}")
        if "commit" in block:
            self.expect(block["commit"] == n.committed, f"HardState commit {n.committed}")
        if "lead_state" in block:
            lead = 0 if n.lead == cs.NONE else n.lead + 1
            self.expect(block["lead_state"] == f"Lead:{lead} State:{STATE_NAME[n.state]}",
                        f"SoftState Lead:{lead} State:{STATE_NAME[n.state]}")
        dummy, ap, u = n.ents[0][0], int(self.be.applied[g]), self.unstable[node]
        ents = ([] if u is None else n.ents[u - dummy:]) + n.ents[ap + 1 - dummy:
                                                                  n.committed + 1 - dummy]
        self.expect([[t, i] for i, t in ents] == block.get("entries", []),
                    f"entries {ents}, the trace {block.get('entries', [])}")
        self.be.applied[g], self.unstable[node] = n.committed, None
        self.checked["readies"] += 1
        hook = HOOKS.get(self.name)
        if hook:
            hook[0](self, node, block)

    def status(self, node, block):
        for k, text in block["progress"].items():
            got = progress_string(self.peer(node, int(k)), self.p.F)
            self.expect(got == text, f"status {k}: {got!r}, the trace {text!r}")
            self.checked["status"] += 1

    # ---- the walk ----
    def run(self):
        p = self.p
        for c in self.cmds:
            if c["line"] < p.start:
                continue
            self.line = c["line"]
            word = c["cmd"].split()
            if word[0] == "campaign":
                self.campaign(int(word[1]))
            elif word[0] in ("propose", "propose-conf-change"):
                self.propose(c)
            elif word[0] == "tick-heartbeat":
                self.tick_heartbeat(int(word[1]))
            elif word[0] == "compact":
                self.fail("`compact` inside the printed part: not driven")
            blocks = c["blocks"]
            if c["line"] == p.start and LEADER_START.get(self.name, {}).get("switch_first"):
                blocks = blocks[LEADER_START[self.name]["skip_blocks"]:]
                self.switch_first()
            for b in blocks:
                node = b.get("node")
                if node is None:
                    node = int(word[1])
                if b["kind"] == "status":
                    self.status(node, b)
                elif b["kind"] == "recv":
                    self.recv(node, b)
                else:
                    self.ready(node, b)
        self.finish()
        return self

    def finish(self):
        self.line = self.cmds[-1]["line"]
        left = [(n, r) for n, rs in self.pending.items() for r in rs]
        self.expect(not left, f"records no Ready showed: {left}")
        sent, received = COUNTS[self.name]
        self.expect(dict(self.sent) == sent, f"sent {dict(self.sent)}, the fixture {sent}")
        self.expect(dict(self.received) == received,
                    f"received {dict(self.received)}, the fixture {received}")
        inflight = Counter(TYPE_NAME[r["type"]] for r in self.pool)
        want = Counter(sent)
        want.subtract(received)
        self.expect(inflight == +want,
                    f"left in flight {dict(inflight)}, the fixture {dict(+want)}")
        self.expect(self.max_runs == self.p.R,
                    f"the run table was filled to {self.max_runs} of {self.p.R} rows")
        hook = HOOKS.get(self.name)
        want = hook[1] if hook else int(bool(LEADER_START.get(self.name, {}).get("switch_first")))
        self.expect(self.switched == want, f"{self.switched} conf switches")


def fmsg(r):
    if r is None:
        return fm.Msg()
    runs = [e for e in (r["ents"] or ()) if e[0]]
    return fm.Msg(r["type"], r["frm"], r["term"], r["index"], r["log_term"], r["commit"], runs)


def vmsg(r):
    if r is None:
        return vm.Msg()
    return vm.Msg(r["type"], r["frm"], r["term"], r["index"], r["log_term"], r["flags"])


def replay(name, **kw):
    """One trace on the model backend -> the Replay (its counters)."""
    tr = traces()[name]
    return Replay(name, tr, TraceModelBackend(params(name, tr), **kw)).run()


if __name__ == "__main__":
    print(f"ALLOWED: {len(ALLOWED)} entries")
    for name in TRACES:
        r = replay(name)
        print(name, dict(r.sent), dict(r.checked), dict(r.be.calls))
