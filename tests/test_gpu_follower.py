"""qe_follower_step on the GPU, bit for bit against tests/follower_model.py:
every state row, every output and the folded statistics after each call, over
the reference's own tables at four tile positions, random states and messages
(logs truncated and regrown over consecutive calls), refused and ignored
groups, sharding; the rows the call has no business with stay untouched; the
response feeds qe_progress_step and the events feed qe_tick as they are."""
import numpy as np
import pytest
import torch

from oracle import orc
from tests import follower_model as fm
from tests import follower_traces as ft
from tests import lift
from tests.golden_util import raft_tables
from tests.test_follower_model import fixture_cases, tables
from tests.test_gpu_progress import DEV, eng  # noqa: F401
from tests.test_progress_oracle import log_runs

pytestmark = pytest.mark.gpu
SENT = 0x0E0E0E0E0E0E0E0E  # prefill: what a call leaves alone keeps it
S8 = SENT & 0xFF
QUIET = ("match", "next", "pending", "peer", "ilo", "ihi", "term_start", "first_index")
SCALARS = ("committed", "last_index", "run_count", "term", "state", "lead", "vote",
           "lead_transferee")
OUT64 = ("resp_index", "reject_hint", "resp_log_term", "append_from")


class Harness:
    """A batch of model nodes resident on the device, with sentinels in every
    row, pad column and output the call must leave alone."""

    def __init__(self, engine, nodes, R, S, stride=None, vote=True, flags=0, goff=0):
        self.e, self.nodes, self.R, self.S, self.flags, self.goff = engine, nodes, R, S, flags, goff
        self.G = len(nodes)
        self.ps = ps = engine.ProgressState(self.G, S, 1, R, DEV, stride=stride, group_offset=goff,
                                            extras=("lead_transferee",))
        self.stride = ps.stride
        for k in QUIET:  # rows of the leader's half
            getattr(ps, k).random_()
        self.quiet = {k: getattr(ps, k).clone() for k in QUIET}
        a = fm.pack_nodes(nodes, R, self.stride, fill=SENT)
        ps.load_host(committed=a["committed"], last_index=a["last_index"],
                     run_first=a["run_first"], run_term=a["run_term"], run_count=a["run_count"],
                     lead_transferee=a["lead_transferee"])
        self.fol = engine.Follower(ps, vote=vote, check_quorum=bool(flags & 1),
                                   prevote=bool(flags & 2))
        self.fol.load_host(term=a["term"], state=a["state"], lead=a["lead"])
        if vote:
            self.fol.load_host(vote=a["vote"])

    def host(self):
        ps, f = self.ps, self.fol.host()
        u64 = lambda t: t.cpu().numpy().view(np.uint64)  # noqa: E731
        h = {"committed": u64(ps.committed), "last_index": u64(ps.last_index),
             "run_first": u64(ps.run_first), "run_term": u64(ps.run_term),
             "run_count": ps.run_count.cpu().numpy(),
             "lead_transferee": ps.lead_transferee.cpu().numpy()}
        h.update(f)
        return h

    def step(self, msgs, E, with_stats=True):
        """One call, compared with the model; -> the model's outs."""
        e, ps, G, R = self.e, self.ps, self.G, self.R
        lm = e.LeaderMsgs(ps, E)
        lm.load_host(**fm.pack_msgs(msgs, E, self.stride))
        out = e.FollowerOut(ps)
        for k in OUT64:
            getattr(out, k).fill_(SENT)
        out.result.fill_(S8)
        out.events.fill_(S8)
        st = e.stats_buffer(DEV) if with_stats else None
        before = self.host()
        assert e.follower_step(ps, self.fol, lm, out, st) is out
        got, o = self.host(), out.host()
        after, outs, stats = fm.step_batch(self.nodes, msgs, self.flags, self.S, R, self.goff)
        want = fm.pack_nodes(after, R, self.stride)
        for k in SCALARS:
            if got[k] is not None:
                np.testing.assert_array_equal(got[k], want[k], err_msg=k)
        touched = np.array([a is not b for a, b in zip(after, self.nodes)])
        cnt = want["run_count"].astype(np.int64)
        for k in ("run_first", "run_term"):
            g2, b2, w2 = (x[k].reshape(R, self.stride) for x in (got, before, want))
            live = np.arange(R)[:, None] < cnt[None, :]
            np.testing.assert_array_equal(g2[:, :G][live], w2[:, :G][live], err_msg=k)
            np.testing.assert_array_equal(g2[:, G:], b2[:, G:], err_msg=k + " pad")
            np.testing.assert_array_equal(g2[:, :G][:, ~touched], b2[:, :G][:, ~touched],
                                          err_msg=k + " of untouched groups")
            # a kept run is never rewritten: rows below the cut keep their bytes
            keep = np.array([len([r for r in n.runs if r[0] < (o_.get("append_from") or 1 << 64)])
                             for n, o_ in zip(self.nodes, outs)])
            kept = np.arange(R)[:, None] < keep[None, :]
            np.testing.assert_array_equal(g2[:, :G][kept], b2[:, :G][kept], err_msg=k + " kept")
        for k in SCALARS:  # an untouched group: not a byte of its state moved
            if got[k] is not None:
                np.testing.assert_array_equal(got[k][~touched], before[k][~touched], err_msg=k)
        for k in QUIET:
            assert torch.equal(getattr(ps, k), self.quiet[k]), k
        np.testing.assert_array_equal(o["result"], [x["result"] for x in outs], err_msg="result")
        np.testing.assert_array_equal(o["events"], [x["events"] for x in outs], err_msg="events")
        for k in OUT64:
            np.testing.assert_array_equal(
                o[k], np.array([x.get(k, SENT) for x in outs], np.uint64), err_msg=k)
        if with_stats:
            folded = e.stats_reduce(st).cpu().numpy().view(np.uint64)
            ws = np.zeros(16, np.uint64)
            for k, v in stats.items():
                ws[k] = v
            np.testing.assert_array_equal(folded, ws, err_msg="stats")
            self.last_stats = folded
        self.nodes = after
        return outs


def neighbours(rng, G, R, S, E):
    nodes = [fm.gen_node(rng, R, S) for _ in range(G)]
    return nodes, [fm.gen_msg(rng, n, E, S) for n in nodes]


def test_fixture_rows_at_four_tile_positions(eng):
    """Every message row of tests/golden/follower_tables.json at lane 0, 63,
    64 and the last lane of a partial tile, among random neighbours."""
    rng = np.random.default_rng(41)
    G, R, S, E = 64 * 2 + 37, 8, 3, 4
    cases = fixture_cases()
    assert len(cases) == 34
    for cid, node, msg in cases:
        nodes, msgs = neighbours(rng, G, R, S, E)
        for pos in (0, 63, 64, G - 1):
            nodes[pos], msgs[pos] = node, msg
        h = Harness(eng, nodes, R, S, flags=int(rng.integers(0, 4)))
        outs = h.step(msgs, E)
        assert len({repr(sorted(outs[p].items())) for p in (0, 63, 64, G - 1)}) == 1, cid


def test_trace_messages_at_four_tile_positions(eng):
    """Every MsgApp / MsgHeartbeat the interaction traces deliver (the
    receiver's state before it as tests/follower_traces.py restates it), four
    trace messages per launch, each at lane 0, 63, 64 and the last lane of
    a partial tile in turn, among random neighbours."""
    rng = np.random.default_rng(43)
    G, R, S, E = 64 * 2 + 37, 8, 7, 4
    spots = (0, 63, 64, G - 1)
    steps, _ = ft.replay_all()
    assert len(steps) == 75
    for k in range(0, len(steps), 4):
        batch = steps[k:k + 4]
        for rot in range(4):
            nodes, msgs = neighbours(rng, G, R, S, E)
            for j, st in enumerate(batch):
                pos = spots[(j + rot) % 4]
                nodes[pos], msgs[pos] = st.before, st.msg
            outs = Harness(eng, nodes, R, S).step(msgs, E)
            for j, st in enumerate(batch):  # the model's answer is the trace's (checked on the CPU)
                assert outs[spots[(j + rot) % 4]] == st.out, st.id


def test_fixture_expectations_on_gpu(eng):
    """The reference's own expected responses, read from the device (the
    model is not in this comparison): TestFollowerCheckMsgApp and the
    follower half of TestFastLogRejection."""
    t = tables()
    rows = []
    for name in ("TestFollowerCheckMsgApp", "TestFastLogRejection"):
        for (cid, node, msg), row in zip([c for c in fixture_cases() if c[0].startswith(name)],
                                         t[name]["rows"]):
            rows.append((node, msg, row))
    h = Harness(eng, [r[0] for r in rows], 8, 3)
    ps = h.ps
    lm = eng.LeaderMsgs(ps, 1)
    lm.load_host(**fm.pack_msgs([r[1] for r in rows], 1, h.stride))
    o = eng.follower_step(ps, h.fol, lm).host()
    for g, (_, _, row) in enumerate(rows):
        rej = o["result"][g] == fm.FR_APP_REJECT
        assert rej == row.get("want_reject", True), g
        if "want_index" in row:
            assert o["resp_index"][g] == row["want_index"], g
        if rej:
            assert (o["reject_hint"][g], o["resp_log_term"][g]) == (row["want_reject_hint"],
                                                                    row["want_log_term"]), g


CASES = [(1, 0, 0, True), (1, 1, 1, False), (1, 4, 2, True),
         (4, 0, 3, False), (4, 1, 0, True), (4, 4, 1, True),
         (16, 0, 2, True), (16, 1, 3, True), (16, 4, 0, False)]


@pytest.mark.parametrize("R,E,flags,vote", CASES)
def test_random_differential(eng, R, E, flags, vote):
    """64 full tiles and a partial one, a stride that is no multiple of
    anything, 8 consecutive calls on the evolving state."""
    rng = np.random.default_rng(7000 + 31 * R + E)
    G, S = 4133, 5
    nodes = [fm.gen_node(rng, R, S) for _ in range(G)]
    h = Harness(eng, nodes, R, S, stride=G + 11, vote=vote, flags=flags, goff=1 << 33)
    seen = set()
    for call in range(8):
        msgs = [fm.gen_msg(rng, n, E, S) for n in h.nodes]
        seen |= {o["result"] for o in h.step(msgs, E)}
    want = {fm.FR_NONE, fm.FR_IGNORED, fm.FR_HEARTBEAT_RESP, fm.FR_APP_ACCEPT, fm.FR_APP_REJECT,
            fm.FR_APP_STALE, fm.FR_BAD_MSG, fm.FR_COMMIT_PAST_LOG}
    want |= {fm.FR_LOWER_TERM_RESP} if flags else set()
    want |= {fm.FR_RUNS_FULL, fm.FR_APP_GAP} if E else set()
    assert want <= seen, sorted(fm.FR_NAMES[c] for c in want - seen)


@pytest.mark.parametrize("case", lift.FOLLOWER_CASES, ids=str)
def test_wide_differential(eng, case):
    """The random differential with every group's indexes and terms lifted
    (tests/lift.py): a base per group out of 0, 2^32 - k, 2^53 + 1, 2^63 - k and
    2^64 - 4096 for each, so the high dword of every state, message and output
    word is live, logs cross the dword boundary and the int64 sign bit.  Nine
    tiles and a ragged one, 8 consecutive calls, statistics on; the model runs
    on the wide values themselves.  tests/test_lift_model.py proves the run's
    coverage on the CPU; it is asserted again on what the device went through."""
    R, E, flags = case
    box = {}

    def stepper(nodes, msgs):
        if not box:
            box["h"] = Harness(eng, nodes, R, lift.FOLLOWER_S, stride=lift.G + lift.PAD,
                               flags=flags, goff=lift.GOFF)
        outs = box["h"].step(msgs, E)
        return box["h"].nodes, outs

    ls, log = lift.follower_run(case, stepper)
    lift.check_follower_coverage(case, ls, log)


def test_top_of_range(eng):
    """2^64 - 1 is QE_INDEX_INF and no log index: the rows of
    lift.follower_top_rows() at lane 0, 63, 64 and the last lane of a partial
    tile among random lifted neighbours.  The harness holds the device to the
    model; the rows' literals hold the model."""
    rng = np.random.default_rng(83)
    G, R, S, E = 64 * 2 + 37, 8, 3, 4
    spots = (0, 63, 64, G - 1)
    results = []
    for row in lift.follower_top_rows():
        nodes, msgs = lift.follower_neighbours(rng, G, R, S, E)
        for pos in spots:
            nodes[pos], msgs[pos] = row[1], row[2]
        h = Harness(eng, nodes, R, S, stride=G + 5, flags=int(rng.integers(0, 4)), goff=1 << 33)
        outs = h.step(msgs, E)
        for pos in spots:
            lift.check_follower_top_row(row, row[1], h.nodes[pos], outs[pos])
        assert len({repr(sorted(outs[p].items())) for p in spots}) == 1, row[0]
        results.append(outs[0]["result"])
    assert results == lift.FOLLOWER_TOP_RESULTS


def test_one_group_and_all_none(eng):
    rng = np.random.default_rng(5)
    for G in (1, 209):
        nodes = [fm.gen_node(rng, 4, 5) for _ in range(G)]
        h = Harness(eng, nodes, 4, 5, stride=G + 3)
        outs = h.step([fm.Msg() for _ in range(G)], 4)  # every group NONE
        assert all(o == {"result": fm.FR_NONE, "events": 0} for o in outs)
        assert not h.last_stats.any()
    h = Harness(eng, [fm.gen_node(rng, 4, 5)], 4, 5, stride=7)
    n = h.nodes[0]
    m = fm.Msg(fm.LMSG_APP, 1, n.term + 1, n.last_index(), n.log_term(n.last_index()),
               n.last_index() + 1, [(1, n.term + 1)])
    assert h.step([m], 1)[0]["result"] in (fm.FR_APP_ACCEPT, fm.FR_RUNS_FULL)
    h.step([m], 1, with_stats=False)  # the same message again, no statistics asked for


def test_refused_and_ignored_groups_change_nothing(eng):
    """One batch of nothing but refusals, lower terms and messages to
    leaders: no state row moves (Harness.step compares every untouched group
    byte for byte with the state before)."""
    rng = np.random.default_rng(11)
    G, R, S = 300, 4, 5
    nodes, msgs = [], []
    for g in range(G):
        n = fm.gen_node(rng, R, S)
        last = n.last_index()
        kind = g % 6
        m = fm.Msg(fm.LMSG_APP, g % S, n.term + 1, last, n.log_term(last), last, [(1, n.term + 1)])
        if kind == 0:
            m.frm = S + g % 7  # BAD_MSG
        elif kind == 1:
            m.type, m.commit = fm.LMSG_HEARTBEAT, last + 1  # COMMIT_PAST_LOG
        elif kind == 2:
            n = fm.Node(n.ents, n.committed, n.term, n.state, n.lead, n.vote, n.transferee)
            m.runs = [(1, n.term + 1 + j) for j in range(R - len(n.runs) + 1)][:4]  # RUNS_FULL
            if len(n.runs) + len(m.runs) <= R:
                m.runs = [(1, 0)]
        elif kind == 3:
            m.index, m.log_term = last + 2, 0  # APP_GAP
        elif kind == 4:
            n.term += 2
            m.term = n.term - 1  # lower term
        else:
            n.state, m.term = fm.ST_LEADER, n.term  # a leader at the message's term
        nodes.append(n)
        msgs.append(m)
    for flags in (0, 3):
        h = Harness(eng, nodes, R, S, flags=flags)
        outs = h.step(msgs, 4)
        assert all(a is b for a, b in zip(h.nodes, nodes))
        res = {o["result"] for o in outs}
        assert res == {fm.FR_BAD_MSG, fm.FR_COMMIT_PAST_LOG, fm.FR_RUNS_FULL, fm.FR_APP_GAP,
                       fm.FR_IGNORED} | ({fm.FR_LOWER_TERM_RESP} if flags else set())


def test_sharding(eng):
    """Two calls over [0, G/2) and [G/2, G) with group_offset give the state
    and the summed statistics of one call."""
    rng = np.random.default_rng(13)
    G, R, S, E = 1001, 4, 5, 4
    nodes, msgs = neighbours(rng, G, R, S, E)
    whole = Harness(eng, nodes, R, S, goff=500)
    whole.step(msgs, E)
    half, total = G // 2, np.zeros(16, np.uint64)
    parts = []
    for lo, hi in ((0, half), (half, G)):
        h = Harness(eng, nodes[lo:hi], R, S, goff=500 + lo)
        h.step(msgs[lo:hi], E)
        total += h.last_stats
        parts.append(h.host())
    np.testing.assert_array_equal(total, whole.last_stats)
    w = whole.host()
    for k in SCALARS:
        np.testing.assert_array_equal(np.concatenate([p[k] for p in parts]), w[k], err_msg=k)


def test_closed_loop_with_progress_step(eng):
    """TestFastLogRejection end to end: the leader's probe goes through
    qe_follower_step, whose response rows are copied into a PeerMsgs as they
    are, and qe_progress_step lands on the next_append_index raft_tables.json
    pins for the leader side."""
    L = orc.lib()
    lrows = raft_tables()["TestFastLogRejection"]["rows"]
    frows = tables()["TestFastLogRejection"]["rows"]
    resp_type = {fm.FR_APP_ACCEPT: 1, fm.FR_APP_REJECT: 2}  # QE_MSG_APP_RESP[_REJECT]
    for lr, fr in zip(lrows, frows):
        lead = [tuple(e) for e in lr["leader_log"]]
        l_last = max(i for i, _ in lead)
        rf, rt, last = log_runs(lead, (l_last + 1, 1))
        ps = eng.ProgressState(1, 1, 16, 16, DEV)
        R = len(rf)
        run_first = np.zeros(16 * ps.stride, np.uint64)
        run_term = np.zeros(16 * ps.stride, np.uint64)
        run_first[np.arange(R) * ps.stride] = rf
        run_term[np.arange(R) * ps.stride] = rt
        ps.load_host(run_first=run_first, run_term=run_term, run_count=np.array([R], np.uint8),
                     first_index=np.array([1], np.uint64), last_index=np.array([last], np.uint64),
                     term_start=np.array([l_last + 1], np.uint64),
                     next=np.array([l_last + 1], np.uint64), match=np.array([0], np.uint64))
        msgs = eng.PeerMsgs(ps)
        msgs.type.fill_(3)  # MsgHeartbeatResp -> the probing MsgApp
        eng.progress_step(ps, msgs)
        probe = int(msgs.msg_index[0])
        assert int(msgs.sent[0]) == 1 and probe == l_last
        # the follower's side of it
        fol_log = [(0, 0)] + [tuple(e) for e in fr["follower_log"]]
        h = Harness(eng, [fm.Node(fol_log, term=0, lead=0)], 8, 1)
        lm = eng.LeaderMsgs(h.ps, 1)
        m = fm.Msg(fm.LMSG_APP, 0, 1, probe, L.orc_log_term(R, orc.P(rf), orc.P(rt), last, probe),
                   0, [(1, 1)])
        lm.load_host(**fm.pack_msgs([m], 1, h.stride))
        out = eng.follower_step(h.ps, h.fol, lm)
        # ... copied as they are
        msgs = eng.PeerMsgs(ps)
        msgs.type[:1].fill_(resp_type[int(out.result[0])])
        msgs.index[:1].copy_(out.resp_index)
        msgs.reject_hint[:1].copy_(out.reject_hint)
        msgs.log_term[:1].copy_(out.resp_log_term)
        eng.progress_step(ps, msgs)
        assert int(msgs.msg_count[0]) == 1
        idx = int(msgs.msg_index[0])
        term = L.orc_log_term(R, orc.P(rf), orc.P(rt), last, idx)
        assert (idx, term) == (lr["next_append_index"], lr["next_append_term"]), lr


def test_events_feed_the_tick(eng):
    """FollowerOut.events handed to tick(..., events=) as it is: a follower
    that heard from its leader does not campaign on that tick, an untouched
    neighbour with the same timer does."""
    G, S, ET = 130, 3, 4
    ps = eng.ProgressState(G, S, 1, 4, DEV, extras=("self_slot",))
    ps.self_slot.zero_()
    ps.run_count.fill_(1)
    t = eng.Timers(G, ET, 1, False, 9, DEV)
    t.load_host(election_elapsed=np.full(G, 2 * ET), randomized_timeout=np.full(G, ET, np.uint16))
    fol = eng.Follower(ps, state=t.state)
    assert fol.state is t.state
    fol.term.fill_(3)
    lm = eng.LeaderMsgs(ps, 0)
    heard = np.zeros(G, bool)
    heard[[0, 63, 64, 129]] = True
    lm.load_host(type=np.where(heard, fm.LMSG_HEARTBEAT, fm.LMSG_NONE).astype(np.uint8),
                 term=np.full(G, 3, np.uint64))
    out = eng.FollowerOut(ps)
    out.events.fill_(S8)  # stale bytes of an earlier use must not survive
    eng.follower_step(ps, fol, lm, out)
    np.testing.assert_array_equal(out.events.cpu().numpy(), np.where(heard, fm.TEV_HEARD, 0))
    act = eng.tick(ps, t, events=out.events).action.cpu().numpy()
    np.testing.assert_array_equal(act & 1, np.where(heard, 0, 1))  # QE_TICK_HUP


def test_walking_waves(eng):
    """One launch in which every wave walks two or three tiles (tests/walk.py):
    the base's 209 groups repeated, statistics on, a group offset past 2^32
    and a stride that is no multiple of 64.  Every row is the base's
    expectation repeated, every counter the repeated base's sum."""
    from tests import walk
    R, S, E = walk.R, walk.S, walk.E
    b = walk.follower_base()
    G = walk.walk_groups(torch.cuda.get_device_properties(DEV).multi_processor_count)
    stride, idx = G + walk.PAD, np.arange(G) % walk.PERIOD
    runs = {"run_first": R, "run_term": R}
    a = walk.repeat(fm.pack_nodes(b.nodes, R, walk.PERIOD), G, stride, runs, fill=SENT)
    ps = eng.ProgressState(G, S, 1, R, DEV, stride=stride, group_offset=walk.GOFF,
                           extras=("lead_transferee",))
    ps.load_host(**{k: a[k] for k in ("committed", "last_index", "run_first", "run_term",
                                      "run_count", "lead_transferee")})
    fol = eng.Follower(ps, check_quorum=bool(b.flags & 1), prevote=bool(b.flags & 2))
    fol.load_host(**{k: a[k] for k in ("term", "state", "lead", "vote")})
    lm = eng.LeaderMsgs(ps, E)
    lm.load_host(**walk.repeat(fm.pack_msgs(b.msgs, E, walk.PERIOD), G, stride,
                               {"ent_len": E, "ent_term": E}))
    out = eng.FollowerOut(ps)
    for k in OUT64:
        getattr(out, k).fill_(SENT)
    out.result.fill_(S8)
    out.events.fill_(S8)
    st = eng.stats_buffer(DEV)
    eng.follower_step(ps, fol, lm, out, st)
    want = walk.repeat(fm.pack_nodes(b.after, R, walk.PERIOD), G, stride, runs, fill=SENT)
    u64 = lambda t: t.cpu().numpy().view(np.uint64)  # noqa: E731
    got = {"committed": u64(ps.committed), "last_index": u64(ps.last_index),
           "run_count": ps.run_count.cpu().numpy(),
           "lead_transferee": ps.lead_transferee.cpu().numpy(), **fol.host()}
    for k in SCALARS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    live = np.arange(R)[:, None] < want["run_count"].astype(np.int64)[None, :]
    for k in runs:
        g2, w2 = u64(getattr(ps, k)).reshape(R, stride), want[k].reshape(R, stride)
        np.testing.assert_array_equal(g2[:, :G][live], w2[:, :G][live], err_msg=k)
        np.testing.assert_array_equal(g2[:, G:], w2[:, G:], err_msg=k + " pad")
    o = out.host()
    res = np.array([x["result"] for x in b.outs], np.uint8)[idx]
    np.testing.assert_array_equal(o["result"], res, err_msg="result")
    np.testing.assert_array_equal(o["events"], np.array([x["events"] for x in b.outs])[idx])
    for k in OUT64:
        np.testing.assert_array_equal(
            o[k], np.array([x.get(k, SENT) for x in b.outs], np.uint64)[idx], err_msg=k)
    folded = eng.stats_reduce(st).cpu().numpy().view(np.uint64)
    ws = walk.expect_stats(b.shares, G, walk.follower_hashes(want, res))
    np.testing.assert_array_equal(folded, ws, err_msg="stats")
    assert ws[fm.STAT_GROUPS] > 0.8 * G and ws[fm.STAT_APPENDED] and ws[fm.STAT_COMMIT_ADVANCED]
