"""tests/trace_cluster.py with the engine beside the models: every node of an
interaction trace is a group of ONE resident batch, and every message a node
steps on was built on the device -- qe_outbox after each leader-side call,
qe_replies after each receiver-side call, on the calls' own device-resident
rows -- and routed on the device by qe_inbox (the rows the step kernels consume
are the tensors qe_inbox filled; the deferred list is gathered on the device).
The records copied back are compared with the reference's printed messages
(tests/golden/interaction_traces.json), field by field, by the same driver as
on the CPU (tests/test_trace_cluster.py proves what it covers).

The backend is tests/test_gpu_inbox_cluster.InboxDeviceBackend, so
DeviceBackend's comparison after every call keeps running beside the trace
comparison: the call's outputs against the models', the whole resident state
against the composed model, and -- byte for byte against the copy taken before
the call -- every row and pad column of the groups without a message.

Shapes: G = 130 groups (two full tiles and a ragged third), stride G + 3,
group_offset 2^33, S = the trace's node count (2, 3 or 7), the run table exactly
as large as the trace needs (campaign.txt: ONE row), the cluster once at groups
[0, S) and once at [61, 61 + S): the 7-node cluster then straddles the 63 | 64
tile edge and its record lists cross it.  Every other group holds a live copy
of the initial state of the node whose slot it falls on and takes no message
(a tick reaches every group; the copies' heartbeat records are not sent).
Both Inflights forms: the 32-bit rings everywhere, the 16-bit form (the one the
benchmark uses) wherever it can hold the trace -- it needs log_runs <= 4, which
rules out probe_and_replicate.txt (five term runs)."""
import time

import numpy as np
import pytest
import torch

from tests import cluster_sim as cs
from tests import outbox_sim as osim
from tests import replies_model as rm
from tests import replies_sim as rsim
from tests import trace_cluster as tc
from tests.test_gpu_cluster import dev_u64
from tests.test_gpu_inbox_cluster import InboxDeviceBackend
from tests.test_gpu_progress import DEV, eng  # noqa: F401
from tests.trace_replay import traces

pytestmark = pytest.mark.gpu
G, GOFF = 130, 1 << 33


class TraceDeviceBackend(tc.TraceHost, InboxDeviceBackend):
    """The engine beside the models on a TraceWorld; `outbox` / `replies` hold
    the DEVICE's records of the calls since the last take()."""

    ready = False

    def __init__(self, engine, p):
        self.outbox, self.replies, self.ob, self.rp = [], [], None, None
        self.listed = 0
        super().__init__(engine, p)
        self.init_trace()
        w, c = self.w, self.conf
        # the configuration is per group here
        for k in ("learner", "is_learner"):
            row = np.array([getattr(x, k) for x in w.confs], np.uint8)
            getattr(c, k).copy_(torch.from_numpy(row).to(DEV).view(getattr(c, k).dtype))
        self.pci_t.copy_(dev_u64(w.pci))  # a leader that leads from the start
        self.ob = self.real.Outbox(self.ps, p.G * p.N, cs.MSG_RUNS)
        self.rp = self.real.Replies(self.ps, p.G * p.N)
        self.ready = True
        self.after(None, [])

    def after(self, touched, outs):
        if not self.ready:  # the rows are not all in place yet
            return []
        return super().after(touched, outs)

    # ---- the record lists, after the call that asks for them ----
    def timed(self, f, *a, **kw):
        e, ps = self.e, self.ps
        nxt0 = ps.next.clone() if f in (e.propose, e.switch_config) else None
        r = super().timed(f, *a, **kw)
        if f is e.progress_step:
            m = a[1]
            self.list_outbox(sent=m.sent, snap=m.snap, index=m.msg_index)
            self.list_replies(timeout_now=m.timeout_now)
        elif f in (e.propose, e.switch_config):
            self.list_outbox(sent=a[1].sent, snap=a[1].snap, next_before=nxt0)
        elif f is e.become_leader:
            ld = a[1]
            won = ld.result == cs.BL_LEADER  # the rows of the others are not outputs
            zero = torch.zeros_like(ld.sent)
            self.list_outbox(sent=torch.where(won, ld.sent, zero),
                             snap=torch.where(won, ld.snap, zero), next_before=ps.next)
        elif f is e.tick:
            o = kw["out"]
            self.list_outbox(hb_sent=o.hb_sent, hb_commit=o.hb_commit, hb_ctx=o.hb_ctx)
        elif f is e.follower_step:
            self.list_replies(follow=(a[2], a[3]))
        elif f is e.snapshot_step:
            self.list_replies(snap=(a[3], a[4]))
        elif f is e.vote_step:
            self.list_replies(vote=(a[3], a[4]))
        return r

    def list_outbox(self, **inp):
        if self.ob is None:
            return
        t0 = time.perf_counter()
        self.real.outbox(self.ps, self.fol.term, self.ob, **inp)
        count, rows = self.ob.records()
        self.gpu_seconds += time.perf_counter() - t0
        assert count <= self.ob.capacity
        for i in range(count):
            r = {k: int(rows[k][i]) for k in ("group", "to", "type", "term", "index", "log_term",
                                              "commit", "ctx")}
            r["ents"] = [(int(rows["ent_len"][j, i]), int(rows["ent_term"][j, i]))
                         for j in range(cs.MSG_RUNS) if rows["ent_len"][j, i]]
            self.outbox.append(r)
        self.listed += count

    def list_replies(self, **inp):
        if self.rp is None:
            return
        t0 = time.perf_counter()
        self.real.replies(self.ps, self.fol.term, self.rp, **inp)
        count, rows = self.rp.records()
        self.gpu_seconds += time.perf_counter() - t0
        assert count <= self.rp.capacity
        self.replies += [{k: int(rows[k][i]) for k in rm.FIELDS} for i in range(count)]
        self.listed += count

    def take(self):
        ob, rp = self.outbox, self.replies
        self.outbox, self.replies = [], []
        osim.by_peer(ob, self.p.goff), rsim.by_key(rp, self.p.goff)  # one per key and call
        return ob, rp

    # ---- the entry points beyond the simulation's ----
    def propose(self, num_entries, cc=None):
        e, ps = self.e, self.ps
        pr = e.Proposals(ps, max_cc=1 if cc else 0)
        pr.num_entries.copy_(torch.from_numpy(num_entries.astype(np.int32)).to(DEV))
        if cc:
            _, cnt, _, lv, _ = self.cc_rows(cc)
            pr.cc_count.copy_(torch.from_numpy(cnt).to(DEV))
            pr.cc_leave.copy_(torch.from_numpy(lv).to(DEV))
        pr.applied.copy_(dev_u64(self.applied))
        pr.pending_conf_index, pr.uncommitted_size = self.pci_t, self.unc_t
        self.timed(e.propose, ps, pr)
        o = self.model_propose(num_entries, cc)
        names = ("result", "sent", "snap", "cc_refused")
        host = self.after(num_entries != 0, [getattr(pr, k) for k in names])
        for k, h in zip(names, host):
            np.testing.assert_array_equal(h, getattr(o, k), err_msg=k)
        return o

    def switch_config(self, switched):
        e, ps = self.e, self.ps
        sw = e.Switch(ps, torch.from_numpy(switched).to(DEV))
        self.timed(e.switch_config, ps, sw)
        o = self.model_switch_config(switched)
        names = ("result", "sent", "snap")
        host = self.after(switched != 0, [getattr(sw, k) for k in names])
        for k, h in zip(names, host):
            np.testing.assert_array_equal(h, getattr(o, k), err_msg=k)
        return o

    def set_conf(self, g, inc, learner):
        """The host's rewrite of one group's masks (the only rows it writes)."""
        super().set_conf(g, inc, learner)
        ps, c = self.ps, self.conf
        ps.inc[g], ps.tracked[g] = inc, inc | learner
        c.learner[g], c.is_learner[g] = learner, learner
        self.prev = None
        self.after(None, [])

    def route(self, recs, tick_action=None, carry=0):
        want = self.model_route(recs, tick_action)
        ents = [list(m["ents"]) for m in recs]
        super().route(recs, tick_action, carry, want)
        for m, x in zip(recs, ents):  # (the upload pads the runs of a record)
            m["ents"] = x
        return want


RING32 = [(name, base, False) for name in tc.TRACES for base in (0, 61)]
RING16 = [(name, 61, True) for name in tc.TRACES if tc.RUNS[name] <= 4]
assert {"snapshot_succeed_via_app_resp.txt", "confchange_v1_remove_leader.txt"} <= \
    {name for name, _, _ in RING16}


@pytest.mark.parametrize("name,base,ring16", RING32 + RING16)
def test_trace_cluster_on_device(eng, name, base, ring16):  # noqa: F811
    tr = traces()[name]
    p = tc.params(name, tr, G=G, gbase=base, goff=GOFF, ring16=ring16)
    assert p.stride == G + 3 and p.R == tc.RUNS[name]
    t0 = time.perf_counter()
    be = TraceDeviceBackend(eng, p)
    r = tc.Replay(name, tr, be).run()
    print(f"{name} base {base} ring16 {ring16}: S {p.N}, R {p.R}, calls "
          f"{sum(be.calls.values())}, inbox passes {be.passes} ({be.gathered} records gathered "
          f"on the device), records {be.listed}, {time.perf_counter() - t0:.2f} s (kernels and "
          f"syncs {be.gpu_seconds:.2f} s), compared {dict(r.checked)}, ALLOWED {len(tc.ALLOWED)}")
    sent, received = tc.COUNTS[name]
    assert dict(r.sent) == sent and dict(r.received) == received
    assert r.checked["records"] == sum(sent.values()) and r.checked["coalesced"] == 0
    ref = tc.Replay(name, tr, tc.TraceModelBackend(p)).run()
    assert r.checked == ref.checked
