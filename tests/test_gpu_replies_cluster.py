"""The closed loop on the receivers' side: tests/test_gpu_cluster.py's
DeviceBackend with qe_replies after every qe_follower_step, qe_snapshot_step,
qe_vote_step and qe_progress_step, on the call's own device-resident rows (the
message rows the call was given, the output rows it wrote, the Follower's term
row after it).  The simulation (tests/replies_sim.py) compares every
MsgAppResp / MsgHeartbeatResp / Msg{Pre}VoteResp / Msg{Pre}Vote its host layer
builds with the device's record, and puts the message REBUILT FROM THE RECORD
on the network: every response and vote message a node steps on was built by
the kernel.  DeviceBackend's own comparison of the whole resident state after
every call keeps running (it also shows that qe_replies wrote none of it).

Rows: "c" as it is and the reduced row "b" of tests/inbox_sim.py (6 clusters of
5, PreVote + CheckQuorum; tests/test_replies_model.py proves on the CPU what
the two show)."""
import time

import pytest

from tests import cluster_sim as cs
from tests import inbox_sim
from tests import replies_model as rm
from tests import replies_sim as rsim
from tests.test_gpu_cluster import DeviceBackend
from tests.test_gpu_progress import eng  # noqa: F401

pytestmark = pytest.mark.gpu


class RepliesDeviceBackend(rsim.ResultLog, DeviceBackend):
    """Every receiver-side call is followed by engine.replies; `self.replies`
    holds the records copied back, {(group, slot, type): record}."""

    def __init__(self, engine, p):
        self.replies, self.rp, self.listed = {}, None, 0
        super().__init__(engine, p)
        # a campaign asks every other slot; a transfer or a response is one record
        self.rp = engine.Replies(self.ps, p.G * p.N)

    def timed(self, f, *a, **kw):
        e = self.e
        r = super().timed(f, *a, **kw)
        if f is e.follower_step:
            self.list_records(follow=(a[2], a[3]))
        elif f is e.snapshot_step:
            self.list_records(snap=(a[3], a[4]))
        elif f is e.vote_step:
            self.list_records(vote=(a[3], a[4]))
        elif f is e.progress_step:
            self.list_records(timeout_now=a[1].timeout_now)
        return r

    def list_records(self, **inp):
        if self.replies:
            raise rsim.RepliesMismatch(f"records no message was built for: {self.replies}")
        t0 = time.perf_counter()
        self.e.replies(self.ps, self.fol.term, self.rp, **inp)
        count, rows = self.rp.records()
        self.gpu_seconds += time.perf_counter() - t0
        assert count <= self.rp.capacity
        recs = [{k: int(rows[k][i]) for k in rm.FIELDS} for i in range(count)]
        self.listed += count
        self.replies = rsim.by_key(recs, self.p.goff)


ROWS = {"c": cs.ROWS["c"], "b_small": cs.ROWS["b"].but(**inbox_sim.ROW_B_SMALL)}


@pytest.mark.parametrize("name", sorted(ROWS))
def test_cluster_runs_on_device_built_replies(eng, name):  # noqa: F811
    p = ROWS[name]
    mbe = rsim.ModelReplies(p)
    ref = rsim.RepliesSim(p, mbe).run()
    t0 = time.perf_counter()
    be = RepliesDeviceBackend(eng, p)
    sim = rsim.RepliesSim(p, be, rebuild=True).run()
    print(f"row {name}: rounds {sim.round_no}, calls {sum(be.calls.values())}, records "
          f"{be.listed}, with the device {time.perf_counter() - t0:.2f} s (kernels and syncs "
          f"{be.gpu_seconds:.2f} s), messages {dict(sim.sent_cov)}")
    assert sim.sent_cov == ref.sent_cov
    for k in rsim.REQUIRED_BY_ROW[name]:
        assert sim.sent_cov[k] > 0, (k, dict(sim.sent_cov))
    assert be.listed == sum(sim.sent_cov.values()) == mbe.listed
    assert sim.counters() == ref.counters()
    assert sim.inv.leaders == ref.inv.leaders
