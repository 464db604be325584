"""The closed loop: tests/test_gpu_cluster.py's DeviceBackend with qe_inbox in
front of every pass of step calls.  The simulation (tests/inbox_sim.py) hands
each pass's list of delivered messages to the device; engine.inbox routes it
into a LeaderMsgs / SnapMsgs / VoteMsgs / PeerMsgs, and THOSE TENSORS are what
qe_follower_step, qe_snapshot_step, qe_progress_step and qe_vote_step consume:
the backend's engine hands them out where DeviceBackend asks for fresh message
rows, and its host upload is dropped (the ConfState of a MsgSnap excepted, which
is the host's by the rules).  From the second pass of a delivery on, the list
is the deferred records gathered on the device (Inbox.gather_deferred) with the
new arrivals behind them.  The rows copied back are compared with
tests/inbox_model.py, and DeviceBackend's comparison of the whole resident
state after every call keeps running (it also shows that qe_inbox wrote none of
it).  With qe_inbox duties H4, H6 and H1's HUP are optional for a host.

Rows: "c" as it is and the reduced row "b" of tests/inbox_sim.py;
tests/test_inbox_model.py proves on the CPU what each shows."""
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import cluster_sim as cs
from tests import inbox_sim as isim
from tests.test_gpu_cluster import DeviceBackend, sentinel
from tests.test_gpu_inbox import arrays, host
from tests.test_gpu_progress import DEV, eng  # noqa: F401

pytestmark = pytest.mark.gpu
PEER_IN = ("type", "index", "reject_hint", "log_term")
ROUTED_ARRAYS = {"lm": ("from_", "term", "index", "log_term", "commit", "ent_len", "ent_term"),
                 "sm": ("from_", "term", "snap_index", "snap_term"),
                 "vm": ("from_", "term", "index", "log_term", "flags")}


class RoutedEngine:
    """The engine, except that the next LeaderMsgs / SnapMsgs / VoteMsgs /
    PeerMsgs asked for is the one qe_inbox filled (`routed`), once each."""

    def __init__(self, e):
        self._e, self.routed = e, {}

    def __getattr__(self, k):
        return getattr(self._e, k)

    def LeaderMsgs(self, ps, msg_runs=1):
        return self.routed.pop("lm", None) or self._e.LeaderMsgs(ps, msg_runs)

    def SnapMsgs(self, ps, ids=False):
        return self.routed.pop("sm", None) or self._e.SnapMsgs(ps, ids)

    def VoteMsgs(self, ps):
        return self.routed.pop("vm", None) or self._e.VoteMsgs(ps)

    def PeerMsgs(self, ps, outputs=True):
        return self.routed.pop("pm", None) or self._e.PeerMsgs(ps, outputs)


def routed_peer_msgs(e, ps):
    """A PeerMsgs whose struct() names the tensors qe_inbox wrote (`routed`);
    the attributes a host upload writes are decoys."""

    class RoutedPeerMsgs(e.PeerMsgs):
        def struct(self):
            decoys = {k: getattr(self, k) for k in PEER_IN}
            self.__dict__.update(self.routed)
            try:
                return super().struct()
            finally:
                self.__dict__.update(decoys)

    pm = RoutedPeerMsgs(ps)
    pm.routed = {k: getattr(pm, k) for k in PEER_IN}
    for k in PEER_IN:
        setattr(pm, k, torch.zeros_like(pm.routed[k]))
    for k in PEER_IN[1:]:
        sentinel(pm.routed[k])
    return pm


class InboxDeviceBackend(DeviceBackend):
    def __init__(self, engine, p):
        super().__init__(RoutedEngine(engine), p)
        self.real = engine
        self.ib = engine.Inbox(self.ps, 4096, cs.MSG_RUNS, ctx=False, flags=True, src=True)
        self.passes = self.records = self.gathered = 0

    def fresh_rows(self):
        e, ps = self.real, self.ps
        lm, sm_, vm_ = e.LeaderMsgs(ps, cs.MSG_RUNS), e.SnapMsgs(ps, ids=True), e.VoteMsgs(ps)
        for obj, kind in ((lm, "lm"), (sm_, "sm"), (vm_, "vm")):
            for k in ROUTED_ARRAYS[kind]:
                sentinel(getattr(obj, k))
        lm.load_host = lambda **a: lm     # what the step kernel reads is what qe_inbox wrote
        vm_.load_host = lambda **a: vm_
        sm_.load_host = lambda **a: e.SnapMsgs.load_host(  # the ConfState is the host's
            sm_, **{k: v for k, v in a.items() if k.startswith("cs_")})
        return lm, sm_, vm_, routed_peer_msgs(e, ps)

    def route(self, recs, tick_action, carry, want):
        """One qe_inbox call on `recs`; its rows must be `want` (the model's)."""
        e, ps, p, ib = self.real, self.ps, self.p, self.ib
        G, N, st, E = p.G, p.N, p.stride, cs.MSG_RUNS
        for m in recs:
            m["ents"] = (m["ents"] + [(0, 0)] * E)[:E]
        t0 = time.perf_counter()
        if carry:  # the deferred records of the pass before, gathered on the device
            assert ib.gather_deferred().n == carry
            ib.load_host(after=carry, **arrays(recs[carry:], E, False, True))
            self.gathered += carry
        else:
            ib.load_host(**arrays(recs, E, False, True))
        lm, sm_, vm_, pm = self.fresh_rows()
        tick_t = None if tick_action is None else torch.from_numpy(tick_action).to(DEV)
        rows = SimpleNamespace(read_ctx=None, **pm.routed)
        e.inbox(ps, self.fol, ib, lm, sm_, vm_, rows, tick_action=tick_t)
        disp, deferred = ib.results()
        self.gpu_seconds += time.perf_counter() - t0
        self.passes, self.records = self.passes + 1, self.records + len(recs)
        # ---- the list the device routed is the list the host holds ----
        if carry:
            for k, v in arrays(recs, E, False, True).items():
                t = getattr(ib, "from_" if k == "from" else k)
                np.testing.assert_array_equal(host(t)[: v.size], v.reshape(-1), err_msg="list " + k)
        # ---- the rows against the model's ----
        eq = np.testing.assert_array_equal
        eq(disp, want.disposition, err_msg="disposition")
        eq(deferred, want.deferred, err_msg="deferred")
        fam = (("f", lm, want.f, dict(frm="from_", term="term", index="index", log_term="log_term",
                                      commit="commit"), ib.f_src),
               ("s", sm_, want.s, dict(frm="from_", term="term", snap_index="snap_index",
                                       snap_term="snap_term"), ib.s_src),
               ("v", vm_, want.v, dict(frm="from_", term="term", index="index",
                                       log_term="log_term", flags="flags"), ib.v_src))
        for name, obj, rows_w, names, src in fam:
            eq(host(obj.type), [rows_w[g]["type"] if g in rows_w else 0 for g in range(G)],
               err_msg=name + "_type")
            gs = sorted(rows_w)
            for k, attr in list(names.items()) + [("src", None)]:
                got = host(src if attr is None else getattr(obj, attr))
                eq(got[gs], np.array([rows_w[g][k] for g in gs], np.uint64).astype(got.dtype),
                   err_msg=f"{name}_{k}")
        el, et = host(lm.ent_len).reshape(E, st), host(lm.ent_term).reshape(E, st)
        for g, r in want.f.items():
            if r["ents"] is not None:
                eq(el[:, g], [x[0] for x in r["ents"]])
                eq(et[:, g], [x[1] for x in r["ents"]])
        rt = host(pm.routed["type"]).reshape(N, st)
        exp = np.zeros((N, st), np.uint8)
        for (s, g), r in want.r.items():
            exp[s, g] = r["type"]
        eq(rt, exp, err_msg="r_type")
        got = {k: host(pm.routed[a]).reshape(N, st) for k, a in
               (("index", "index"), ("hint", "reject_hint"), ("log_term", "log_term"))}
        got["src"] = host(ib.r_src).reshape(N, st)
        for (s, g), r in want.r.items():
            assert all(int(got[k][s, g]) == r[k] for k in got), ("r", s, g, r)
        self.e.routed = dict(lm=lm, sm=sm_, vm=vm_, pm=pm)


class DeviceInboxSim(isim.InboxSim):
    """InboxSim whose routing runs on the device; the model's result is what
    the device's rows are held against, and what drives the simulation."""

    def route(self, recs, tick_action):
        want = super().route(recs, tick_action)
        self.be.route(recs, tick_action, self.carry, want)
        return want


ROWS = {"c": cs.ROWS["c"], "b_small": cs.ROWS["b"].but(**isim.ROW_B_SMALL)}


@pytest.mark.parametrize("name", sorted(ROWS))
def test_cluster_runs_on_device_routed_rows(eng, name):  # noqa: F811
    p = ROWS[name]
    ref = isim.InboxSim(p, cs.ModelBackend(p)).run()
    t0 = time.perf_counter()
    be = InboxDeviceBackend(eng, p)
    sim = DeviceInboxSim(p, be).run()
    print(f"row {name}: rounds {sim.round_no}, calls {sum(be.calls.values())}, inbox passes "
          f"{be.passes} over {be.records} records ({be.gathered} gathered on the device), with "
          f"the device {time.perf_counter() - t0:.2f} s (kernels and syncs {be.gpu_seconds:.2f} "
          f"s), kinds {dict(sim.kinds)}, dispositions {dict(sim.dispositions)}")
    assert sim.kinds == ref.kinds and sim.dispositions == ref.dispositions
    for k in isim.REQUIRED_BY_ROW[name]:
        assert sim.kinds[k] > 0, (k, dict(sim.kinds))
    assert be.gathered > 0
    assert sim.counters() == ref.counters()
    assert sim.inv.leaders == ref.inv.leaders
