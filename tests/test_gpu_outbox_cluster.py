"""The closed loop: tests/test_gpu_cluster.py's DeviceBackend with qe_outbox
after every leader-side call, on the call's own device-resident output rows
(qe_progress_step's sent / snap / msg_index, qe_propose's and
qe_become_leader's sent / snap with Next, qe_tick's hb_sent / hb_commit /
hb_ctx).  The simulation (tests/outbox_sim.py) compares every MsgApp / MsgSnap /
MsgHeartbeat its host layer builds with the device's record, and puts the
message REBUILT FROM THE RECORD on the network: every such message a follower
steps on was built by the kernel.  DeviceBackend's own comparison of the whole
resident state after every call keeps running (it also shows that qe_outbox
wrote none of it).

Rows: "c" as it is (one cluster, log_runs 16) and the reduced row "a" of
tests/outbox_sim.py (6 clusters, log_runs 8; tests/test_outbox_model.py proves
on the CPU that it shows every kind of message)."""
import time

import pytest
import torch

from tests import cluster_sim as cs
from tests import outbox_sim as osim
from tests.test_gpu_cluster import DeviceBackend
from tests.test_gpu_progress import eng  # noqa: F401

pytestmark = pytest.mark.gpu


class OutboxDeviceBackend(DeviceBackend):
    """Every leader-side call is followed by engine.outbox; `self.outbox` holds
    the records copied back, {(group, slot): record}."""

    def __init__(self, engine, p):
        self.outbox, self.ob, self.listed = {}, None, 0
        super().__init__(engine, p)
        self.ob = engine.Outbox(self.ps, p.G * p.N, cs.MSG_RUNS)

    def timed(self, f, *a, **kw):
        e, ps = self.e, self.ps
        nxt0 = ps.next.clone() if f is e.propose else None  # Next before the call
        r = super().timed(f, *a, **kw)
        if f is e.progress_step:
            m = a[1]
            self.list_records(sent=m.sent, snap=m.snap, index=m.msg_index)
        elif f is e.propose:
            self.list_records(sent=a[1].sent, snap=a[1].snap, next_before=nxt0)
        elif f is e.become_leader:
            ld = a[1]
            won = ld.result == cs.BL_LEADER  # the rows of the others are not outputs
            zero = torch.zeros_like(ld.sent)
            self.list_records(sent=torch.where(won, ld.sent, zero),
                              snap=torch.where(won, ld.snap, zero), next_before=ps.next)
        elif f is e.tick:
            o = kw["out"]
            self.list_records(hb_sent=o.hb_sent, hb_commit=o.hb_commit, hb_ctx=o.hb_ctx)
        return r

    def list_records(self, **inp):
        if self.outbox:
            raise osim.OutboxMismatch(f"records no message was built for: {self.outbox}")
        t0 = time.perf_counter()
        self.e.outbox(self.ps, self.fol.term, self.ob, **inp)
        count, rows = self.ob.records()
        self.gpu_seconds += time.perf_counter() - t0
        assert count <= self.ob.capacity
        recs = []
        for i in range(count):
            r = {k: int(rows[k][i]) for k in ("group", "to", "type", "term", "index", "log_term",
                                              "commit", "ctx")}
            r["ents"] = [(int(rows["ent_len"][j, i]), int(rows["ent_term"][j, i]))
                         for j in range(cs.MSG_RUNS) if rows["ent_len"][j, i]]
            recs.append(r)
        self.listed += count
        self.outbox = osim.by_peer(recs, self.p.goff)


ROWS = {"c": cs.ROWS["c"], "a_small": cs.ROWS["a"].but(**osim.ROW_A_SMALL)}


@pytest.mark.parametrize("name", sorted(ROWS))
def test_cluster_runs_on_device_built_messages(eng, name):  # noqa: F811
    p = ROWS[name]
    ref = osim.OutboxSim(p, osim.ModelOutbox(p)).run()
    t0 = time.perf_counter()
    be = OutboxDeviceBackend(eng, p)
    sim = osim.OutboxSim(p, be, rebuild=True).run()
    print(f"row {name}: rounds {sim.round_no}, calls {sum(be.calls.values())}, records "
          f"{be.listed}, with the device {time.perf_counter() - t0:.2f} s (kernels and syncs "
          f"{be.gpu_seconds:.2f} s), messages {dict(sim.sent_cov)}")
    assert sim.sent_cov == ref.sent_cov
    want = osim.REQUIRED if name == "a_small" else ("snap", "app_two_runs", "app_empty",
                                                    "heartbeat")
    for k in want:
        assert sim.sent_cov[k] > 0, (k, dict(sim.sent_cov))
    assert be.listed == sim.sent_cov["app"] + sim.sent_cov["snap"] + sim.sent_cov["heartbeat"]
    assert sim.counters() == ref.counters()
    assert sim.inv.leaders == ref.inv.leaders
