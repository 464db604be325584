"""tests/cluster_sim.py with the engine beside the models: every entry point
(qe_tick, qe_vote_step, qe_follower_step, qe_snapshot_step, qe_compact,
qe_become_leader, qe_propose, qe_progress_step) writes to ONE resident state in
which every row has meaning, under a lossy, duplicating, reordering,
partitioning network.  After every call the call's outputs are compared bit for
bit with the model's and the whole resident state with the composed model:
every row of every family, the pad columns, and -- byte for byte against the
copy taken before the call -- everything of the groups without a message.
After every round the Raft invariants (cluster_sim.Invariants) run on the rows
copied back from the device, not on the models.  The coverage counters must be
the CPU run's of the same seed (tests/test_cluster_model.py proves what they
cover): the same schedule ran.

Rows (cluster_sim.ROWS): a -- 66 clusters of 3 (G = 198), log_runs 4, the 16-bit
Inflights form with cap 4, every index crossing 2^32; b -- 27 clusters of 5
(G = 135), log_runs 8, 32-bit rings with cap 2, PreVote + CheckQuorum,
group_offset 2^33, slot 4 a learner (the masks go through as they are: no new
engine work); c -- one cluster of 3, log_runs 16, CheckQuorum, 32-bit rings
(the 16-bit form requires log_runs <= 4)."""
import time

import numpy as np
import pytest
import torch

from tests import cluster_sim as cs
from tests import follower_model as fm
from tests import snapshot_model as sm
from tests import tick_model as tm
from tests import vote_model as vm
from tests.test_gpu_progress import (DEV, RING_MASK, assert_same, eng, live_entries,  # noqa: F401
                                     load_msgs)

pytestmark = pytest.mark.gpu
SENT = 0x0E0E0E0E0E0E0E0E  # prefill: what a call leaves alone keeps it
S8 = SENT & 0xFF
PW_PAD = 0x000E0E0E        # a pad peer word without ring representation bits


def dev_u64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to(DEV)


def sentinel(t):
    t.view(torch.uint8).fill_(S8)
    return t


class DeviceBackend(cs.ModelBackend):
    """The model backend with every call made on the device too."""

    def __init__(self, engine, p):
        super().__init__(p)
        self.e = e = engine
        w, pb, G, N, st = self.w, self.w.pb, p.G, p.N, p.stride
        pad = np.arange(N * st).reshape(N, st)[:, G:].reshape(-1)
        for k in ("match", "next", "pending"):
            getattr(pb, k)[pad] = SENT
        pb.pw[pad] = PW_PAD
        self.ps = ps = e.ProgressState(
            G, N, p.F, p.R, DEV, masks=("inc",), group_offset=p.goff, stride=st,
            extras=("tracked", "self_slot", "lead_transferee", "snap_index", "reads"),
            ring16=p.ring16)
        assert ps.stride == st
        md = cs.orc.mask_dtype(N)
        runs = {k: np.full(p.R * st, SENT, np.uint64) for k in ("run_first", "run_term")}
        for g, n in enumerate(w.nodes):
            for r, (f, t) in enumerate(n.runs):
                runs["run_first"][r * st + g], runs["run_term"][r * st + g] = f, t
        ps.load_host(match=pb.match, next=pb.next, pending=pb.pending, peer=pb.pw, ibuf=pb.ibuf,
                     committed=pb.committed, term_start=pb.term_start,
                     first_index=pb.first_index, last_index=pb.last_index,
                     run_count=pb.run_count, inc=pb.inc, tracked=pb.tracked,
                     self_slot=pb.self_slot, lead_transferee=pb.lead_transferee,
                     snap_index=pb.snap_index, read_acks=pb.read_acks.view(md),
                     read_head=pb.read_head, read_count=pb.read_count, **runs)
        cq, pv = bool(p.flags & vm.VOTE_CHECK_QUORUM), bool(p.flags & vm.VOTE_PREVOTE)
        self.t = t = e.Timers(G, p.ET, 1, cq, p.seed, DEV)
        t.load_host(randomized_timeout=w.tm.rt.astype(np.uint16))
        self.fol = fol = e.Follower(ps, state=t.state, check_quorum=cq, prevote=pv)
        a = vm.pack_nodes(w.nodes, p.R, N, st)
        fol.load_host(term=a["term"], state=a["state"], lead=a["lead"], vote=a["vote"])
        self.voter = e.Voter(ps, timers=t, prevote=pv)
        self.voter.load_host(voted=a["voted"], granted=a["granted"])
        # the ConfState restore writes: its inc / tracked ARE the rows qe_vote_step,
        # qe_tick and the leader's kernels read
        self.conf = c = e.ConfState(G, N, DEV)
        c.inc, c.tracked = ps.inc, ps.tracked
        c.learner.fill_(w.learner)
        c.is_learner.fill_(w.learner)
        ids = np.array([[s + 1] * G for s in range(N)], np.uint64).reshape(-1)
        c.slot_ids.copy_(dev_u64(ids))
        self.pci_t = torch.zeros(G, dtype=torch.int64, device=DEV)
        self.unc_t = torch.zeros(G, dtype=torch.int64, device=DEV)
        self.events_t = self.elected_t = self.elected_np = None
        self.gpu_seconds = 0.0
        # every resident tensor and how groups index it
        self.rows = [(k, getattr(ps, k), "ks") for k in
                     ("match", "next", "pending", "peer", "run_first", "run_term")]
        self.rows += [(k, getattr(ps, k), "ksx") for k in ("ilo", "ihi", "infl16")
                      if getattr(ps, k) is not None]
        self.rows += [(k, getattr(ps, k), "g") for k in
                      ("committed", "term_start", "first_index", "last_index", "run_count", "inc",
                       "tracked", "self_slot", "lead_transferee", "snap_index", "read_head",
                       "read_count")]
        self.rows += [("read_acks", ps.read_acks, "gx")]
        self.rows += [(k, getattr(fol, k), "g") for k in ("term", "state", "lead", "vote")]
        self.rows += [(k, getattr(self.voter, k), "g") for k in ("voted", "granted")]
        self.rows += [("t_" + k, getattr(t, k), "g") for k in
                      ("timer", "randomized_timeout", "no_campaign")]
        self.rows += [("c_" + k, getattr(c, k), "g") for k in
                      ("out", "learner", "learners_next", "is_learner", "auto_leave")]
        self.rows += [("c_slot_ids", c.slot_ids, "kg"), ("pci", self.pci_t, "g"),
                      ("unc", self.unc_t, "g")]
        assert_same(ps, pb)
        self.prev = None
        self.after(None, [])

    # ---- the comparison after every call ----
    NP = {torch.int64: np.uint64, torch.int32: np.uint32, torch.int16: np.uint16,
          torch.uint8: np.uint8}

    def fetch(self, tensors):
        """The tensors as numpy arrays (unsigned views) in ONE device-to-host
        copy (wide element types first, so every view is aligned)."""
        order = sorted(range(len(tensors)), key=lambda i: -tensors[i].element_size())
        flat = torch.cat([tensors[i].reshape(-1).view(torch.uint8) for i in order]).cpu().numpy()
        out, o = [None] * len(tensors), 0
        for i in order:
            t = tensors[i]
            n = t.numel() * t.element_size()
            out[i] = flat[o:o + n].view(self.NP[t.dtype])
            o += n
        return out

    def untouched_equal(self, cur, touched):
        """Everything of the groups without a message (and every pad column),
        byte for byte against the state after the call before."""
        p = self.p
        G, st = p.G, p.stride
        keep = np.ones(st, bool)
        keep[:G] = ~touched
        kg = keep[:G]
        for name, _, lay in self.rows:
            a, b = cur[name], self.prev[name]
            if lay == "g":
                ok = (a[kg] == b[kg]).all()
            elif lay == "ks":
                ok = (a.reshape(-1, st)[:, keep] == b.reshape(-1, st)[:, keep]).all()
            elif lay == "ksx":
                ok = (a.reshape(p.N, st, -1)[:, keep] == b.reshape(p.N, st, -1)[:, keep]).all()
            elif lay == "gx":
                ok = (a.reshape(G, -1)[kg] == b.reshape(G, -1)[kg]).all()
            else:
                ok = (a.reshape(-1, G)[:, kg] == b.reshape(-1, G)[:, kg]).all()
            assert ok, name + ": a group without a message (or a pad column) changed"

    def rings(self, cur):
        """Every ring position decoded to uint64, entry-major [S][F][stride]
        (ProgressState.rings on the rows already copied back)."""
        ps, L = self.ps, self.e._lib.lib()
        S, F, st = ps.S, ps.F, ps.stride
        ent = np.zeros(S * st * F, np.uint64)
        a = {k: np.ascontiguousarray(cur[k]) for k in ("ilo", "ihi", "peer", "next")}
        if ps.infl16 is not None:
            o16 = np.ascontiguousarray(cur["infl16"])
            rc = L.qe_ring_unpack16(ps.G, S, F, st, o16.ctypes.data, a["ilo"].ctypes.data,
                                    a["ihi"].ctypes.data, a["next"].ctypes.data,
                                    a["peer"].ctypes.data, ent.ctypes.data)
        else:
            rc = L.qe_ring_unpack(ps.G, S, F, st, a["ilo"].ctypes.data, a["ihi"].ctypes.data,
                                  a["peer"].ctypes.data, ent.ctypes.data)
        assert rc == 0
        return np.ascontiguousarray(ent.reshape(S, st, F).transpose(0, 2, 1)).reshape(-1)

    def after(self, touched, outs):
        """After a call (the model has stepped too): the whole resident state
        against the composed model and, for the groups without a message,
        against its bytes before the call.  -> `outs` (tensors) as numpy."""
        p, w = self.p, self.w
        G, N, st, R = p.G, p.N, p.stride, p.R
        got = self.fetch([t for _, t, _ in self.rows] + list(outs))
        cur = {name: a for (name, _, _), a in zip(self.rows, got)}
        if self.prev is not None:
            self.untouched_equal(cur, touched)
        self.prev = cur
        eq = np.testing.assert_array_equal
        pb = w.pb
        # the leader half, as test_gpu_progress.assert_same holds it
        for k in ("match", "next", "pending", "committed", "lead_transferee", "read_head",
                  "read_count", "term_start", "first_index", "last_index", "snap_index",
                  "run_count", "self_slot", "inc", "tracked"):
            eq(cur[k], getattr(pb, k), err_msg=k)
        eq(cur["read_acks"], pb.read_acks.view(cs.orc.mask_dtype(N)), err_msg="read_acks")
        eq(cur["peer"] & ~RING_MASK, pb.pw, err_msg="packed peer words")
        live = live_entries(pb.pw, N, p.F, st)
        eq(self.rings(cur)[live], pb.ibuf[live], err_msg="live ring entries")
        # the log, the follower rows, the Votes
        want = vm.pack_nodes(w.nodes, R, N, st)
        live = np.arange(R)[:, None] < want["run_count"].astype(np.int64)[None, :]
        for k in ("run_first", "run_term"):
            eq(cur[k].reshape(R, st)[:, :G][live], want[k].reshape(R, st)[:, :G][live], err_msg=k)
        for k in ("term", "state", "lead", "vote", "voted", "granted"):
            eq(cur[k], want[k], err_msg=k)
        # the timers
        eq(cur["t_timer"], w.tm.timer(), err_msg="timer")
        eq(cur["t_randomized_timeout"], w.tm.rt.astype(np.uint16), err_msg="randomized_timeout")
        assert not cur["t_no_campaign"].any()
        # the configuration (inc / tracked are the leader half's rows above)
        for k in ("out", "learner", "learners_next", "is_learner", "auto_leave"):
            eq(cur["c_" + k], [getattr(c, k) for c in w.confs], err_msg="c_" + k)
        eq(cur["inc"], [c.inc for c in w.confs], err_msg="c_inc")
        eq(cur["tracked"], [c.tracked for c in w.confs], err_msg="c_tracked")
        eq(cur["c_slot_ids"].reshape(N, G).T, [c.ids for c in w.confs], err_msg="c_slot_ids")
        eq(cur["pci"], w.pci, err_msg="pending_conf_index")
        eq(cur["unc"], w.unc, err_msg="uncommitted_size")
        return got[len(self.rows):]

    def timed(self, f, *a, **kw):
        t0 = time.perf_counter()
        r = f(*a, **kw)
        torch.cuda.synchronize()
        self.gpu_seconds += time.perf_counter() - t0
        return r

    def check_outs(self, names, host, outs, sentinels):
        """host: the output rows in the order of `names`; a row the call does
        not write for a group keeps its sentinel."""
        for k, got in zip(names, host):
            sent = sentinels.get(k)
            want = [o[k] for o in outs] if sent is None else [o.get(k, sent) for o in outs]
            np.testing.assert_array_equal(got, np.array(want, got.dtype), err_msg=k)

    # ---- one method per entry point ----
    def tick(self, events, ticks):
        e, ps, p = self.e, self.ps, self.p
        G, N, st = p.G, p.N, p.stride
        ev = None if events is None else self.events_t  # as it lies on the device
        out = e.TickOut(ps)
        for k in ("hb_commit", "hb_ctx", "quorum_active"):
            sentinel(getattr(out, k))
        self.timed(e.tick, ps, self.t, out=out, events=ev, ticks=ticks)
        mo = super().tick(events, ticks)
        touched = np.ones(G, bool) if ticks else np.asarray(events) != 0
        extra = [] if ev is None else [ev]
        act, sent, hc, ctx, qa, *evh = self.after(
            touched, [out.action, out.hb_sent, out.hb_commit, out.hb_ctx, out.quorum_active] + extra)
        if evh:  # the events the simulation routed are the device's row
            np.testing.assert_array_equal(evh[0], events, err_msg="events")
        np.testing.assert_array_equal(act, mo.action, err_msg="action")
        np.testing.assert_array_equal(sent, mo.hb_sent, err_msg="hb_sent")
        to = (mo.hb_sent[None, :].astype(np.int64) >> np.arange(N)[:, None] & 1) != 0
        hc = hc.reshape(N, st)
        np.testing.assert_array_equal(hc[:, :G][to], mo.hb_commit.reshape(N, st)[:, :G][to])
        assert (hc[:, :G][~to] == SENT).all() and (hc[:, G:] == SENT).all()
        beat, chk = (mo.action & tm.BEAT) != 0, (mo.action & tm.CHECKED_QUORUM) != 0
        np.testing.assert_array_equal(ctx[beat], mo.hb_ctx[beat], err_msg="hb_ctx")
        assert (ctx[~beat] == SENT & 0xFFFFFFFF).all()
        np.testing.assert_array_equal(qa[chk], mo.quorum_active[chk], err_msg="quorum_active")
        assert (qa[~chk] == S8).all()
        return mo

    def clear_lead(self, groups):
        super().clear_lead(groups)
        self.fol.lead[torch.tensor(groups, device=DEV)] = 0xFF
        self.prev["lead"] = self.prev["lead"].copy()
        self.prev["lead"][groups] = 0xFF

    def vote(self, msgs):
        e, ps, N = self.e, self.ps, self.p.N
        vmsg = e.VoteMsgs(ps)
        vmsg.load_host(**vm.pack_msgs(msgs))
        out = e.VoteOut(ps)
        for k in out.ARRAYS:
            sentinel(getattr(out, k))
        self.timed(e.vote_step, ps, self.fol, self.voter, vmsg, out)
        outs = super().vote(msgs)
        host = self.after(np.array([m.type != 0 for m in msgs]),
                          [getattr(out, k) for k in out.ARRAYS])
        mask = SENT & (0xFF if N <= 8 else 0xFFFF)
        self.check_outs(out.ARRAYS, host, outs,
                        {"resp_term": SENT, "req_log_term": SENT, "req_to": mask})
        self.events_t, self.elected_t = out.events, out.elected
        self.elected_np = np.array([o["elected"] for o in outs], np.uint8)
        return outs

    def follow(self, msgs):
        e, ps, p = self.e, self.ps, self.p
        lm = e.LeaderMsgs(ps, cs.MSG_RUNS)
        lm.load_host(**fm.pack_msgs(msgs, cs.MSG_RUNS, p.stride))
        out = e.FollowerOut(ps)
        for k in out.ARRAYS:
            sentinel(getattr(out, k))
        self.timed(e.follower_step, ps, self.fol, lm, out)
        outs = super().follow(msgs)
        host = self.after(np.array([m.type != 0 for m in msgs]),
                          [getattr(out, k) for k in out.ARRAYS])
        self.check_outs(out.ARRAYS, host, outs,
                        {"resp_index": SENT, "append_from": SENT, "reject_hint": SENT,
                         "resp_log_term": SENT})
        self.events_t = out.events
        return outs

    def snap(self, msgs):
        e, ps, p = self.e, self.ps, self.p
        smg = e.SnapMsgs(ps, ids=True)
        smg.load_host(**sm.pack_smsgs(msgs, p.N, p.stride))
        out = e.SnapOut(ps)
        for k in out.ARRAYS:
            sentinel(getattr(out, k))
        self.timed(e.snapshot_step, ps, self.fol, self.conf, smg, out)
        outs = super().snap(msgs)
        host = self.after(np.array([m.type != 0 for m in msgs]),
                          [getattr(out, k) for k in out.ARRAYS])
        self.check_outs(out.ARRAYS, host, outs, {"resp_index": SENT})
        self.events_t = out.events
        return outs

    def compact(self, reqs):
        e, ps = self.e, self.ps
        cp = e.Compaction(ps)
        cp.load_host(compact_index=np.array([r[0] for r in reqs], np.uint64),
                     create_index=np.array([r[1] for r in reqs], np.uint64),
                     applied=np.array([r[2] for r in reqs], np.uint64))
        sentinel(cp.result), sentinel(cp.snap_term)
        self.timed(e.compact, ps, cp)
        outs = super().compact(reqs)
        host = self.after(np.array([bool(r[0] or r[1]) for r in reqs]), [cp.result, cp.snap_term])
        self.check_outs(("result", "snap_term"), host, outs, {"snap_term": SENT})
        return outs

    def become_leader(self, elected):
        e, ps = self.e, self.ps
        if self.elected_np is not None and np.array_equal(elected, self.elected_np):
            el = self.elected_t  # VoteOut.elected as it lies on the device
        else:                    # the retry after QE_BL_RUNS_FULL
            el = torch.from_numpy(np.ascontiguousarray(elected, np.uint8)).to(DEV)
        ld = e.Leader(ps, el, bcast=True)
        ld.term = self.fol.term
        for k in ("pending_conf_index", "uncommitted_size", "sent", "snap"):
            sentinel(getattr(ld, k))
        self.timed(e.become_leader, ps, ld)
        o = super().become_leader(elected)
        won = o.result == cs.BL_LEADER
        wt = torch.from_numpy(won).to(DEV)
        self.pci_t.copy_(torch.where(wt, ld.pending_conf_index, self.pci_t))
        self.unc_t.copy_(torch.where(wt, ld.uncommitted_size, self.unc_t))
        names = ("result", "sent", "snap", "pending_conf_index", "uncommitted_size")
        host = self.after(np.asarray(elected) != 0, [getattr(ld, k) for k in names])
        np.testing.assert_array_equal(host[0], o.result, err_msg="result")
        for k, h in zip(names[1:], host[1:]):
            np.testing.assert_array_equal(h[won], getattr(o, k)[won], err_msg=k)
        return o

    def propose(self, num_entries):
        e, ps = self.e, self.ps
        pr = e.Proposals(ps)
        pr.num_entries.copy_(torch.from_numpy(num_entries.astype(np.int32)).to(DEV))
        pr.pending_conf_index, pr.uncommitted_size = self.pci_t, self.unc_t
        self.timed(e.propose, ps, pr)
        o = super().propose(num_entries)
        names = ("result", "sent", "snap")
        host = self.after(num_entries != 0, [getattr(pr, k) for k in names])
        for k, h in zip(names, host):
            np.testing.assert_array_equal(h, getattr(o, k), err_msg=k)
        return o

    def progress_step(self, mtype, mindex, mhint, mlogterm):
        e, ps, p = self.e, self.ps, self.p
        msgs = load_msgs(e, ps, mtype, mindex, mhint, mlogterm)
        self.timed(e.progress_step, ps, msgs)
        o = super().progress_step(mtype, mindex, mhint, mlogterm)
        names = ("sent", "snap", "timeout_now", "bcast", "msg_count", "msg_index",
                 "read_released", "term_commit", "term_commit_index")
        h = dict(zip(names, self.after(mtype.reshape(p.N, p.stride)[:, : p.G].any(0),
                                       [getattr(msgs, k) for k in names])))
        eq = np.testing.assert_array_equal  # as test_gpu_progress.assert_outputs
        for k in ("sent", "snap", "timeout_now", "bcast", "msg_count", "read_released",
                  "term_commit"):
            eq(h[k], getattr(o, k), err_msg=k)
        cnt, tc = h["msg_count"] > 0, h["term_commit"] > 0
        eq(h["msg_index"][cnt], o.msg_index[cnt], err_msg="msg_index")
        eq(h["term_commit_index"][tc], o.term_commit_index[tc], err_msg="term_commit_index")
        return o

    def view(self):
        """The plain per-node state from the device rows copied back."""
        p, cur = self.p, self.prev  # the rows as the last call's copy holds them
        R, st = p.R, p.stride
        term, state, rc = cur["term"], cur["state"], cur["run_count"]
        com, first, last = cur["committed"], cur["first_index"], cur["last_index"]
        rf, rt = cur["run_first"].reshape(R, st), cur["run_term"].reshape(R, st)
        return [{"term": int(term[g]), "state": int(state[g]), "committed": int(com[g]),
                 "first_index": int(first[g]), "last_index": int(last[g]),
                 "runs": [(int(rf[r, g]), int(rt[r, g])) for r in range(int(rc[g]))]}
                for g in range(p.G)]


@pytest.mark.parametrize("name", sorted(cs.ROWS))
def test_cluster(eng, name):
    """One row of cluster_sim.ROWS: bit-exact after every call, the invariants
    on the device rows after every round, convergence after the heal, the
    coverage list, and the CPU run's counters at the same seed."""
    p = cs.ROWS[name]
    t0 = time.perf_counter()
    ref = cs.Sim(p, cs.ModelBackend(p)).run()
    t1 = time.perf_counter()
    be = DeviceBackend(eng, p)
    sim = cs.Sim(p, be).run()
    t2 = time.perf_counter()
    print(f"row {name}: rounds {sim.round_no}, calls {sum(be.calls.values())}, model-only "
          f"{t1 - t0:.2f} s, with the device {t2 - t1:.2f} s (kernels and syncs "
          f"{be.gpu_seconds:.2f} s), discards {dict(sim.discards)}")
    assert cs.missing(name, sim.cov) == []
    assert sim.counters() == ref.counters()
    assert sim.inv.leaders == ref.inv.leaders
