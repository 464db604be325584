"""qe_vote_step on the GPU, bit for bit against tests/vote_model.py: every
state row, every output and the folded statistics after each call, over the
reference's own tables and trace messages at four tile positions, random
states and messages of all seven types (votes stick and terms climb over
consecutive calls), voter-only and full launches, tiles with no message,
sharding, the argument checks, and the closed loop qe_tick -> qe_vote_step ->
qe_become_leader -> qe_follower_step on clusters whose nodes are groups of one
batch.  The rows the call has no business with (the log, the Progress rows,
the rings, the configuration, the timers) stay byte-identical."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from tests import follower_model as fm
from tests import lift
from tests import tick_model as tm
from tests import vote_model as vm
from tests import vote_traces as vt
from tests.test_gpu_progress import DEV, eng  # noqa: F401
from tests.test_vote_model import _msg, _node, fixture_cases, tables

pytestmark = pytest.mark.gpu
SENT = 0x0E0E0E0E0E0E0E0E  # prefill: what a call leaves alone keeps it
S8 = SENT & 0xFF
PAD = 64  # sentinel elements before and after every row the call may write
QUIET = ("match", "next", "pending", "peer", "ilo", "ihi", "term_start", "first_index",
         "committed", "last_index", "run_count", "run_first", "run_term", "inc", "out", "tracked",
         "self_slot")
STATE = ("term", "state", "lead", "vote", "lead_transferee", "voted", "granted")
LOG = ("committed", "last_index", "run_count")
OUTS = ("result", "resp_term", "req_log_term", "req_to", "elected", "events")


def padded(t):
    """-> (the whole buffer, a view of it with PAD sentinel elements on both sides)."""
    big = torch.empty(t.numel() + 2 * PAD, dtype=t.dtype, device=t.device)
    big.view(torch.uint8).fill_(S8)
    view = big[PAD:PAD + t.numel()]
    view.copy_(t)
    return big, view


def pads_intact(big):
    b = big.view(torch.uint8)
    k = PAD * big.element_size()
    return bool((b[:k] == S8).all()) and bool((b[-k:] == S8).all())


def _np(t):
    a = t.cpu().numpy()
    return a.view({np.dtype(np.int64): np.uint64, np.dtype(np.int32): np.uint32,
                   np.dtype(np.int16): np.uint16}.get(a.dtype, a.dtype))


class Harness:
    """A batch of model nodes resident on the device, with sentinels in every
    row, pad and output the call must leave alone.  With `timers` the state
    and timer rows are the Timers' (the closed loop); else they are private
    and padded."""

    def __init__(self, engine, nodes, R, S, stride=None, flags=0, goff=0, cand=True,
                 have_self=True, et=10, timers=None, F=1):
        self.e, self.nodes, self.R, self.S, self.flags, self.goff = engine, nodes, R, S, flags, goff
        self.cand, self.have_self, self.et, self.timers = cand, have_self, et, timers
        self.G = G = len(nodes)
        masks = tuple(k for k in ("inc", "out") if getattr(nodes[0], k) is not None)
        extras = ("lead_transferee",) + (("self_slot",) if have_self else ()) + \
            (("tracked",) if nodes[0].tracked is not None else ())
        self.ps = ps = engine.ProgressState(G, S, F, R, DEV, masks=masks, group_offset=goff,
                                            stride=stride, extras=extras)
        self.stride = ps.stride
        if timers is None:  # rows of the leader's half: any bytes
            for k in QUIET[:8]:
                getattr(ps, k).random_()
        a = vm.pack_nodes(nodes, R, S, self.stride, fill=SENT)
        ps.load_host(**{k: a[k] for k in ("committed", "last_index", "run_first", "run_term",
                                          "run_count", "lead_transferee", "inc", "out", "tracked")})
        if have_self:
            ps.load_host(self_slot=a["self_slot"])
        self.fol = engine.Follower(ps, state=None if timers is None else timers.state)
        self.fol.load_host(term=a["term"], state=a["state"], lead=a["lead"], vote=a["vote"])
        self.voter = engine.Voter(ps, timers=timers, votes=cand, check_quorum=bool(flags & 1),
                                  prevote=bool(flags & 2), election_timeout=et)
        if timers is None:
            self.voter.timer = torch.from_numpy(a["timer"].view(np.int32)).to(DEV)
            self.voter.no_campaign = torch.from_numpy(a["no_campaign"]).to(DEV)
        if cand:
            self.voter.load_host(voted=a["voted"], granted=a["granted"])
        self.bigs = {}
        if timers is None:
            for obj, names in ((self.fol, ("term", "state", "lead", "vote")),
                               (ps, ("lead_transferee",)), (self.voter, ("voted", "granted"))):
                for k in names:
                    if getattr(obj, k) is not None:
                        self.bigs[k], view = padded(getattr(obj, k))
                        setattr(obj, k, view)

    def host(self):
        ps, v = self.ps, self.voter
        h = {"term": _np(self.fol.term), "state": _np(self.fol.state), "lead": _np(self.fol.lead),
             "vote": _np(self.fol.vote), "lead_transferee": _np(ps.lead_transferee),
             "voted": None if v.voted is None else _np(v.voted),
             "granted": None if v.granted is None else _np(v.granted),
             "committed": _np(ps.committed), "last_index": _np(ps.last_index),
             "run_count": _np(ps.run_count), "run_first": _np(ps.run_first),
             "run_term": _np(ps.run_term)}
        return h

    def quiet(self):
        q = {k: getattr(self.ps, k).clone() for k in QUIET if getattr(self.ps, k) is not None}
        q["timer"] = self.voter.timer.clone()
        q["no_campaign"] = self.voter.no_campaign.clone()
        return q

    def compare_state(self, after, before=None, touched=None):
        """The device rows against the model's nodes (and, for the groups the
        model did not touch, against the bytes before)."""
        got, R, G = self.host(), self.R, self.G
        want = vm.pack_nodes(after, R, self.S, self.stride)
        for k in STATE + LOG:
            if got[k] is None:
                continue
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)
            if before is not None:
                np.testing.assert_array_equal(got[k][~touched], before[k][~touched], err_msg=k)
        live = np.arange(R)[:, None] < want["run_count"].astype(np.int64)[None, :]
        for k in ("run_first", "run_term"):
            g2, w2 = (x[k].reshape(R, self.stride)[:, :G] for x in (got, want))
            np.testing.assert_array_equal(g2[live], w2[live], err_msg=k)
        return got

    def step(self, msgs, with_stats=True):
        """One call, compared with the model; -> the model's outs."""
        e, ps, G, S = self.e, self.ps, self.G, self.S
        vmsg = e.VoteMsgs(ps)
        vmsg.load_host(**vm.pack_msgs(msgs))
        out = e.VoteOut(ps)
        obig = {}
        for k in OUTS:
            obig[k], view = padded(getattr(out, k))
            view.view(torch.uint8).fill_(S8)
            setattr(out, k, view)
        st = e.stats_buffer(DEV) if with_stats else None
        before, quiet = self.host(), self.quiet()
        assert e.vote_step(ps, self.fol, self.voter, vmsg, out, st) is out
        after, outs, stats = vm.step_batch(self.nodes, msgs, self.flags, S, self.et, self.cand,
                                           self.have_self, self.goff)
        touched = np.array([a is not b for a, b in zip(after, self.nodes)])
        self.compare_state(after, before, touched)
        for k, v in self.quiet().items():  # the log, the Progress rows, the rings, the timers
            assert torch.equal(v, quiet[k]), k
        for k, big in list(self.bigs.items()) + list(obig.items()):
            assert pads_intact(big), k
        o = out.host()
        for k in ("result", "events", "elected"):
            np.testing.assert_array_equal(o[k], [x[k] for x in outs], err_msg=k)
        sent_mask = SENT & (0xFF if S <= 8 else 0xFFFF)
        for k, sent in (("resp_term", SENT), ("req_log_term", SENT), ("req_to", sent_mask)):
            np.testing.assert_array_equal(
                o[k], np.array([x.get(k, sent) for x in outs], o[k].dtype), err_msg=k)
        self.out = out
        if with_stats:
            folded = e.stats_reduce(st).cpu().numpy().view(np.uint64)
            ws = np.zeros(16, np.uint64)
            for k, v in stats.items():
                ws[k] = v
            np.testing.assert_array_equal(folded, ws, err_msg="stats")
            self.last_stats = folded
        self.nodes = after
        return outs


SPOTS = lambda G: (0, 63, 128, G - 1)  # noqa: E731  first lane, lane 63, tile 2, last live lane
G3 = 197  # three full tiles and a ragged one


def neighbours(rng, G, R, S, masks="inc"):
    nodes = [vm.gen_node(rng, R, S, masks) for _ in range(G)]
    return nodes, [vm.gen_msg(rng, n, S) for n in nodes]


def test_fixture_rows_at_four_tile_positions(eng):
    """Every row of tests/golden/vote_tables.json and every message of the
    traces' elections at the first lane, lane 63, the first lane of tile 2 and
    the last live lane, among random neighbours; the model's answer there is
    the one the CPU tests hold against the reference's expectation."""
    rng = np.random.default_rng(41)
    cases = [(cid, S, flags, et, node, msg) for cid, S, flags, et, node, msg, _ in fixture_cases()]
    steps, _ = vt.replay_all()
    cases += [(s.id, vt.S, 0, 10, s.before, s.msg) for s in steps]
    assert len(cases) == 74 + 21
    for cid, S, flags, et, node, msg in cases:
        nodes, msgs = neighbours(rng, G3, 8, S)
        for pos in SPOTS(G3):
            nodes[pos], msgs[pos] = node, msg
        h = Harness(eng, nodes, 8, S, flags=flags, et=et, stride=G3 + 5)
        outs = h.step(msgs)
        assert len({repr(sorted(outs[p].items())) for p in SPOTS(G3)}) == 1, cid
        want, _ = vm.step(node, msg, flags, S, et)
        assert all(h.nodes[p].key() == want.key() for p in SPOTS(G3)), cid


def test_fixture_expectations_on_gpu(eng):
    """The reference's expected responses read from the device (the model is
    not in this comparison): every table row in one launch per table."""
    for name, t in tables().items():
        rows = t.get("cases", [])
        if not rows:
            continue
        S, flags, et = t["num_slots"], t["flags"], t.get("election_timeout", 10)
        h = Harness(eng, [_node(c["node"]) for c in rows], 8, S, flags=flags, et=et)
        vmsg = eng.VoteMsgs(h.ps)
        vmsg.load_host(**vm.pack_msgs([_msg(c["msg"]) for c in rows]))
        o = eng.vote_step(h.ps, h.fol, h.voter, vmsg).host()
        got = h.host()
        for g, c in enumerate(rows):
            want = c["want"]
            if want["response"] is None:
                assert o["result"][g] == vm.VR_IN_LEASE, (name, g)
            else:
                assert o["result"][g] == (vm.VR_REJECT if want["response"]["reject"]
                                          else vm.VR_GRANT), (name, g)
                if "term" in want["response"]:
                    assert o["resp_term"][g] == want["response"]["term"], (name, g)
            for k in ("term", "vote", "state"):
                if k in want:
                    assert got[k][g] == want[k], (name, g, k)


def test_election_in_one_round_on_gpu(eng):
    """TestLeaderElectionInOneRoundRPC's response sequences, each at the four
    tile positions, the neighbours stepping random messages meanwhile."""
    rng = np.random.default_rng(47)
    t = tables()["TestLeaderElectionInOneRoundRPC"]
    S = t["num_slots"]
    for seq in t["sequences"]:
        nodes, msgs = neighbours(rng, G3, 4, S)
        for pos in SPOTS(G3):
            nodes[pos], msgs[pos] = _node(seq["node"]), vm.Msg(vm.VMSG_HUP)
        h = Harness(eng, nodes, 4, S)
        h.step(msgs)
        for r in seq["responses"]:
            msgs = [vm.gen_msg(rng, n, S) for n in h.nodes]
            for pos in SPOTS(G3):
                msgs[pos] = vm.Msg(vm.VMSG_VOTE_RESP, r["from"], h.nodes[pos].term,
                                   flags=vm.VMF_REJECT if r["reject"] else 0)
            h.step(msgs)
        for pos in SPOTS(G3):
            assert (h.nodes[pos].state, h.nodes[pos].term) == (seq["want"]["state"],
                                                               seq["want"]["term"])


def run_on_device(engine, case):
    """vote_model.random_run with every call made on the device too."""
    S, R, masks, flags, cand, have_self = case
    box = {}

    def stepper(nodes, msgs):
        if not box:
            box["h"] = Harness(engine, nodes, R, S, stride=vm.RUN_G + 14, flags=flags,
                               goff=vm.RUN_GOFF, cand=cand, have_self=have_self)
        outs = box["h"].step(msgs)
        return box["h"].nodes, outs

    return vm.random_run(case, stepper)


@pytest.mark.parametrize("case", vm.RUN_CASES, ids=str)
def test_random_differential(eng, case):
    """Three full tiles and a ragged one, a stride > G, a group offset past 2^32,
    all seven message types and four flag combinations, 8 consecutive calls on
    one state; voter-only launches and a launch without self_slot refuse the
    candidate's messages.  (That the run meets every result code is asserted
    on the CPU, tests/test_vote_model.py.)"""
    assert run_on_device(eng, case) == vm.random_run(case)


@pytest.mark.parametrize("case", vm.RUN_CASES, ids=str)
def test_wide_differential(eng, case):
    """The eight run cases with every group's indexes and terms lifted
    (tests/lift.py): the term preamble, isUpToDate's (lastTerm, lastIndex)
    compare and term + 1 of a campaign on words whose high dword is live, that
    cross 2^32 inside a log and that pass the int64 sign bit.  Nine tiles and a
    ragged one, 8 calls, statistics on; the model runs on the wide values.
    Per term base the run meets every result code tests/test_vote_model.py
    proves for the small run (on the CPU in tests/test_lift_model.py, and
    asserted here on what the device went through)."""
    S, R, masks, flags, cand, have_self = case
    box = {}

    def stepper(nodes, msgs):
        if not box:
            box["h"] = Harness(eng, nodes, R, S, stride=lift.G + lift.PAD, flags=flags,
                               goff=lift.GOFF, cand=cand, have_self=have_self)
        outs = box["h"].step(msgs)
        return box["h"].nodes, outs

    ls, log = lift.vote_run(case, stepper)
    lift.check_vote_coverage(case, ls, log)


def test_tile_with_no_message(eng):
    """A tile whose groups all have QE_VMSG_NONE, between two tiles with
    messages, and a launch with no message at all: only result / events /
    elected are written (Harness.step holds every other byte)."""
    rng = np.random.default_rng(5)
    for quiet_tiles in ((1,), (0, 1, 2, 3)):
        nodes, msgs = neighbours(rng, G3, 4, 5)
        for g in range(G3):
            if g // 64 in quiet_tiles:
                msgs[g] = vm.Msg()
        h = Harness(eng, nodes, 4, 5, stride=G3 + 3)
        outs = h.step(msgs)
        for g in range(G3):
            if g // 64 in quiet_tiles:
                assert outs[g] == {"result": vm.VR_NONE, "events": 0, "elected": 0}
        if len(quiet_tiles) == 4:
            assert not h.last_stats.any()
        h.step(msgs, with_stats=False)


def test_sharding(eng):
    """Two calls over [0, G/2) and [G/2, G) with group_offset give the state
    and the summed statistics (the checksum) of one call."""
    rng = np.random.default_rng(13)
    S, R = 5, 4
    nodes, msgs = neighbours(rng, G3, R, S)
    whole = Harness(eng, nodes, R, S, goff=500, flags=3)
    whole.step(msgs)
    half, total, parts = 96, np.zeros(16, np.uint64), []
    for lo, hi in ((0, half), (half, G3)):
        h = Harness(eng, nodes[lo:hi], R, S, goff=500 + lo, flags=3)
        h.step(msgs[lo:hi])
        total += h.last_stats
        parts.append(h.host())
    np.testing.assert_array_equal(total, whole.last_stats)
    w = whole.host()
    for k in STATE + LOG:
        np.testing.assert_array_equal(np.concatenate([p[k] for p in parts]), w[k], err_msg=k)


def test_argument_checks(eng):
    """Every QE_EINVAL row of the header, and num_groups == 0."""
    L, lib = eng._lib.lib(), eng._lib
    rng = np.random.default_rng(3)
    nodes = [vm.gen_node(rng, 4, 5, "joint") for _ in range(70)]
    h = Harness(eng, nodes, 4, 5, flags=1)
    vmsg, out = eng.VoteMsgs(h.ps), eng.VoteOut(h.ps)
    out.result.fill_(S8)

    def call(edit=None, null=None):
        s = {"p": h.ps.struct(), "f": h.fol.struct(), "v": h.voter.struct(), "m": vmsg.struct(),
             "o": out.struct()}
        if edit:
            edit(s)
        a = [None if null == k else C.byref(s[k]) for k in ("p", "f", "v", "m", "o")]
        return L.qe_vote_step(*a, None, None)

    def setter(which, field, value=None):
        return lambda s: setattr(s[which], field, value)

    assert call() == lib.QE_OK
    assert (out.result != S8).all()
    for k in ("p", "f", "v", "m", "o"):
        assert call(null=k) == lib.QE_EINVAL, k
    nulls = [("o", "result"), ("f", "term"), ("f", "state"), ("f", "lead"), ("f", "vote"),
             ("m", "type"), ("m", "from_"), ("m", "term"), ("m", "index"), ("m", "log_term"),
             ("p", "last_index"), ("p", "run_term"), ("p", "run_first"), ("p", "run_count"),
             ("v", "timer"),    # QE_VOTE_CHECK_QUORUM without timer
             ("p", "inc_mask"),  # out_mask without inc_mask
             ("v", "voted"), ("v", "granted")]  # exactly one of them
    for which, field in nulls:
        assert call(setter(which, field)) == lib.QE_EINVAL, (which, field)
    for which, field, value in (("v", "election_timeout", 0), ("v", "election_timeout", 32769),
                                ("v", "flags", 4), ("v", "flags", 0x80000001),
                                ("p", "log_runs", 0), ("p", "log_runs", 17),
                                ("p", "stride", 69)):
        assert call(setter(which, field, value)) == lib.QE_EINVAL, (which, field, value)
    # what is optional stays optional
    assert call(setter("v", "election_timeout", 32768)) == lib.QE_OK
    assert call(setter("m", "flags")) == lib.QE_OK
    assert call(setter("v", "no_campaign")) == lib.QE_OK

    def voter_only(s):
        s["v"].voted = s["v"].granted = None
    assert call(voter_only) == lib.QE_OK
    for k in ("resp_term", "req_log_term", "req_to", "elected", "events"):
        assert call(setter("o", k)) == lib.QE_OK, k
    # num_groups == 0: QE_OK and nothing is written
    out.result.fill_(S8)
    assert call(setter("p", "num_groups", 0)) == lib.QE_OK
    assert (out.result == S8).all()


# ---------------------------------------------------------------------------
# The closed loop.  The routing below is test code, not engine logic: it plays
# the host that carries messages between the nodes of a cluster.
# ---------------------------------------------------------------------------
class Cluster:
    """C clusters of N nodes; node i of cluster c is group c * N + i and sits
    in slot i.  The device state and the model (vote_model nodes, the tick
    model) are driven in lockstep and compared after every call."""

    ET = 4

    def __init__(self, engine, C_, N, flags, seed):
        self.e, self.C, self.N, self.flags = engine, C_, N, flags
        self.G = G = C_ * N
        self.R = 8
        cq = bool(flags & vm.VOTE_CHECK_QUORUM)
        nodes = [vm.Node([(0, 0), (1, 1), (2, 1)], committed=2, term=1, self_slot=g % N)
                 for g in range(G)]
        self.t = engine.Timers(G, self.ET, 1, cq, seed, DEV)
        self.h = Harness(engine, nodes, self.R, N, flags=flags, et=self.ET, timers=self.t, F=8)
        self.m = tm.Model(G, N, self.ET, 1, cq, seed=seed, stride=self.h.stride)
        self.m.self_slot = np.array([g % N for g in range(G)], np.uint8)
        self.m.lead_transferee = np.full(G, 0xFF, np.uint8)
        # staggered first timeouts (the same draw everywhere would make every
        # first election a split vote)
        rt = np.random.default_rng(seed).integers(self.ET, 2 * self.ET, G)
        self.t.load_host(randomized_timeout=rt.astype(np.uint16))
        self.m.rt[:] = rt
        self.leaders = {}  # (cluster, term) -> slot
        self.results = set()

    # ---- the timers ----
    def tick(self, events, ticks):
        e, h, m = self.e, self.h, self.m
        ps = h.ps
        m.state[:] = [n.state for n in h.nodes]
        m.peer[:], m.match[:], m.committed[:] = _np(ps.peer), _np(ps.match), _np(ps.committed)
        out = e.tick(ps, self.t, events=events, ticks=ticks)
        mo = m.tick(None if events is None else events.cpu().numpy(), ticks=ticks)
        th = self.t.host()
        np.testing.assert_array_equal(th["timer"], m.timer(), err_msg="timer")
        np.testing.assert_array_equal(th["randomized_timeout"], m.rt.astype(np.uint16))
        np.testing.assert_array_equal(th["state"], m.state)
        np.testing.assert_array_equal(out.action.cpu().numpy(), mo.action, err_msg="action")
        # no leader sits through an election timeout in this test
        assert not (mo.action & (tm.STEPDOWN | tm.CHECKED_QUORUM)).any()
        for g, n in enumerate(h.nodes):
            n.elapsed = int(m.ee[g])
        return out, mo

    def settle(self, events):
        """The events of a call applied before the next one reads the timers
        (the lease precondition): qe_tick with ticks == 0."""
        self.tick(events, 0)

    # ---- one call of each kind ----
    def vote(self, msgs):
        outs = self.h.step(msgs)
        self.results |= {o["result"] for o in outs}
        self.settle(self.h.out.events)
        return outs

    def follow(self, msgs):
        e, h = self.e, self.h
        lm = e.LeaderMsgs(h.ps, 1)
        lm.load_host(**fm.pack_msgs(msgs, 1, h.stride))
        out = e.follower_step(h.ps, h.fol, lm)
        after, outs, _ = fm.step_batch(h.nodes, msgs, 0, self.N, self.R)
        np.testing.assert_array_equal(out.result.cpu().numpy(), [o["result"] for o in outs])
        np.testing.assert_array_equal(out.events.cpu().numpy(), [o["events"] for o in outs])
        h.compare_state(after)
        h.nodes = after
        self.settle(out.events)
        return outs

    def lead(self, elected):
        """qe_become_leader with VoteOut.elected and the Follower's term row
        as they are; the model appends the new term's empty entry."""
        e, h = self.e, self.h
        ld = e.Leader(h.ps, elected, bcast=True)
        ld.term = h.fol.term
        e.become_leader(h.ps, ld)
        res = ld.result.cpu().numpy()
        el = elected.cpu().numpy()
        np.testing.assert_array_equal(res, np.where(el != 0, 1, 0))  # QE_BL_LEADER
        prev = {}
        for g in np.flatnonzero(el):
            n = h.nodes[g] = copy.deepcopy(h.nodes[g])
            last = n.last_index()
            prev[g] = (last, n.log_term(last))
            n.ents.append((last + 1, n.term))
            if n.runs[-1][1] != n.term:
                n.runs.append((last + 1, n.term))
            n.check()
            key = (g // self.N, n.term)
            assert key not in self.leaders, key  # at most one leader per term
            self.leaders[key] = g % self.N
        h.compare_state(h.nodes)
        return prev

    # ---- a tick and everything it sets off ----
    def round(self):
        N, h = self.N, self.h
        _, mo = self.tick(None, 1)
        none = lambda: [vm.Msg() for _ in range(self.G)]  # noqa: E731
        # the leaders' beats reach the other nodes of their clusters
        beat = np.flatnonzero(mo.action & tm.BEAT)
        hc = mo.hb_commit.reshape(N, h.stride)
        for s in sorted({g % N for g in beat}):
            msgs = [fm.Msg() for _ in range(self.G)]
            for g in beat:
                if g % N == s:
                    for i in range(N):
                        if i != s:
                            msgs[g - s + i] = fm.Msg(fm.LMSG_HEARTBEAT, s, h.nodes[g].term,
                                                     commit=int(hc[i, g]))
            self.follow(msgs)
        hup = np.flatnonzero(mo.action & tm.HUP)
        if not len(hup):
            return
        msgs = none()
        for g in hup:
            msgs[g] = vm.Msg(vm.VMSG_HUP)
        campaigns = self.campaigns(self.vote(msgs))
        assert len(campaigns) == len(hup)
        while campaigns:
            # requests: one call per sender slot, so duelling candidates of a
            # cluster are heard in slot order
            responses = []
            for s in range(N):
                msgs, any_ = none(), False
                for g, o in campaigns:
                    if g % N != s:
                        continue
                    ty = vm.VMSG_VOTE if o["result"] == vm.VR_CAMPAIGN_VOTE else vm.VMSG_PREVOTE
                    for i in range(N):
                        if o["req_to"] >> i & 1:
                            msgs[g - s + i] = vm.Msg(ty, s, o["resp_term"], o["last_index"],
                                                     o["req_log_term"])
                            any_ = True
                if not any_:
                    continue
                for g2, o2 in enumerate(self.vote(msgs)):
                    r = vt.response_of(o2)
                    if r is not None:
                        responses.append((g2 - g2 % N + s, g2 % N, msgs[g2].type + 2, r))
            # responses: one call per responding slot
            campaigns, elected = [], torch.zeros(self.G, dtype=torch.uint8, device=DEV)
            for s in range(N):
                msgs = none()
                mine = [x for x in responses if x[1] == s]
                if not mine:
                    continue
                for to, frm, ty, (rej, term) in mine:
                    msgs[to] = vm.Msg(ty, frm, term, flags=vm.VMF_REJECT if rej else 0)
                outs = self.vote(msgs)
                campaigns += self.campaigns(outs)
                elected |= h.out.elected
            if bool(elected.any()):
                prev = self.lead(elected)
                # the new leaders' first MsgApp on the other nodes
                for s in sorted({g % N for g in prev}):
                    msgs = [fm.Msg() for _ in range(self.G)]
                    for g, (pi, pt) in prev.items():
                        if g % N == s:
                            n = h.nodes[g]
                            for i in range(N):
                                if i != s:
                                    msgs[g - s + i] = fm.Msg(fm.LMSG_APP, s, n.term, pi, pt,
                                                             n.committed, [(1, n.term)])
                    self.follow(msgs)

    def campaigns(self, outs):
        got = []
        for g, o in enumerate(outs):
            if o["result"] in (vm.VR_CAMPAIGN_VOTE, vm.VR_CAMPAIGN_PREVOTE):
                got.append((g, dict(o, last_index=self.h.nodes[g].last_index())))
        return got


@pytest.mark.parametrize("C_,N,flags", [(43, 3, 0), (25, 5, vm.VOTE_PREVOTE | vm.VOTE_CHECK_QUORUM)])
def test_closed_loop(eng, C_, N, flags):
    """qe_tick until some QE_TICK_HUP -> qe_vote_step (HUP) -> the requests
    routed by req_to -> the responses routed back -> qe_become_leader on
    VoteOut.elected -> one qe_follower_step of the leader's first MsgApp ->
    the events into the next qe_tick; every row compared after every call."""
    cl = Cluster(eng, C_, N, flags, seed=77 + N)
    for _ in range(2 * Cluster.ET - 1):  # every node's timeout passes once; no leader's does
        cl.round()
    assert cl.leaders, "no cluster elected a leader"
    assert {vm.VR_GRANT, vm.VR_REJECT, vm.VR_WON} <= cl.results
    assert N == 3 or vm.VR_PENDING in cl.results  # (two of three is a quorum at once)
    want = vm.VR_CAMPAIGN_PREVOTE if flags & vm.VOTE_PREVOTE else vm.VR_CAMPAIGN_VOTE
    assert want in cl.results
    # at most one leader per cluster and term (asserted as they were elected);
    # the device agrees with the model on who leads now
    state = _np(cl.h.fol.state)
    for c in range(C_):
        lead = [i for i in range(N) if state[c * N + i] == vm.ST_LEADER]
        terms = {cl.h.nodes[c * N + i].term for i in lead}
        assert len(terms) == len(lead), (c, lead)


def test_walking_waves(eng):
    """One candidate-form launch in which every wave walks two or three tiles
    (tests/walk.py): the base's 209 groups repeated, statistics on, a group
    offset past 2^32 and a stride that is no multiple of 64.  Every row is the
    base's expectation repeated, every counter the repeated base's sum."""
    from tests import walk
    R, S = walk.R, walk.S
    b = walk.vote_base()
    G = walk.walk_groups(torch.cuda.get_device_properties(DEV).multi_processor_count)
    stride, idx = G + walk.PAD, np.arange(G) % walk.PERIOD
    runs = {"run_first": R, "run_term": R}
    a = walk.repeat(vm.pack_nodes(b.nodes, R, S, walk.PERIOD), G, stride, runs, fill=SENT)
    ps = eng.ProgressState(G, S, 1, R, DEV, masks=("inc",), group_offset=walk.GOFF, stride=stride,
                           extras=("lead_transferee", "self_slot", "tracked"))
    ps.load_host(**{k: a[k] for k in ("committed", "last_index", "run_first", "run_term",
                                      "run_count", "lead_transferee", "inc", "tracked",
                                      "self_slot")})
    fol = eng.Follower(ps)
    fol.load_host(**{k: a[k] for k in ("term", "state", "lead", "vote")})
    voter = eng.Voter(ps, check_quorum=bool(b.flags & 1), prevote=bool(b.flags & 2),
                      election_timeout=b.et)
    voter.timer = torch.from_numpy(a["timer"].view(np.int32)).to(DEV)
    voter.no_campaign = torch.from_numpy(a["no_campaign"]).to(DEV)
    voter.load_host(voted=a["voted"], granted=a["granted"])
    vmsg = eng.VoteMsgs(ps)
    vmsg.load_host(**walk.repeat(vm.pack_msgs(b.msgs), G, stride))
    out = eng.VoteOut(ps)
    for k in OUTS:
        getattr(out, k).view(torch.uint8).fill_(S8)
    st = eng.stats_buffer(DEV)
    log_before = {k: getattr(ps, k).clone() for k in ("run_first", "run_term") + LOG}
    eng.vote_step(ps, fol, voter, vmsg, out, st)
    want = walk.repeat(vm.pack_nodes(b.after, R, S, walk.PERIOD), G, stride, runs, fill=SENT)
    got = {"term": _np(fol.term), "state": _np(fol.state), "lead": _np(fol.lead),
           "vote": _np(fol.vote), "lead_transferee": _np(ps.lead_transferee),
           "voted": _np(voter.voted), "granted": _np(voter.granted)}
    for k in STATE:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    for k, v in log_before.items():  # the log is read only
        assert torch.equal(getattr(ps, k), v), k
    o = out.host()
    res = np.array([x["result"] for x in b.outs], np.uint8)[idx]
    ev = np.array([x["events"] for x in b.outs], np.uint8)[idx]
    np.testing.assert_array_equal(o["result"], res, err_msg="result")
    np.testing.assert_array_equal(o["events"], ev, err_msg="events")
    np.testing.assert_array_equal(o["elected"], np.array([x["elected"] for x in b.outs])[idx])
    for k, sent in (("resp_term", SENT), ("req_log_term", SENT), ("req_to", S8)):
        np.testing.assert_array_equal(
            o[k], np.array([x.get(k, sent) for x in b.outs], o[k].dtype)[idx], err_msg=k)
    folded = eng.stats_reduce(st).cpu().numpy().view(np.uint64)
    ws = walk.expect_stats(b.shares, G, walk.vote_hashes(want, res, ev))
    np.testing.assert_array_equal(folded, ws, err_msg="stats")
    assert ws[vm.STAT_GROUPS] > 0.8 * G and ws[vm.STAT_LEADERS] and ws[vm.STAT_STEPDOWNS]
