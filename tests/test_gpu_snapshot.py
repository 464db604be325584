"""qe_snapshot_step and qe_compact on the GPU, bit for bit against
tests/snapshot_model.py: every state row, every configuration row, every
output and the folded statistics after each call, over the reference's own
tables and the traces' MsgSnap deliveries at four tile positions, random states
(compact -> restore -> compact on the same rows), a sparse batch, the argument
checks, and the closed loop compact -> MsgSnap -> restore -> MsgAppResp ->
Replicate -> MsgApp with the leader's and the follower's kernels.

Results no random batch can produce: none -- every QE_SR_* and QE_CP_* code is
generated (test_random_differential asserts it)."""
import ctypes as C

import numpy as np
import pytest
import torch

from etcd_amd import _lib
from tests import follower_model as fm
from tests import lift
from tests import snapshot_model as sm
from tests.test_gpu_progress import DEV, eng  # noqa: F401
from tests.test_snapshot_model import compaction_cases, fixture_cases, storage, trace_cases

pytestmark = pytest.mark.gpu
SENT = 0x0E0E0E0E0E0E0E0E  # prefill: what a call leaves alone keeps it
S8 = SENT & 0xFF
QUIET = ("match", "next", "pending", "peer", "ilo", "ihi", "term_start")
LOG = ("committed", "last_index", "run_count", "first_index", "snap_index", "self_slot",
       "lead_transferee")
FOL = ("term", "state", "lead", "vote")
CONF = tuple("c_" + k for k in sm.CONF_MASKS) + ("c_auto_leave", "c_slot_ids")


def u64(t):
    return t.cpu().numpy().view(np.uint64)


class Harness:
    """A batch of model nodes resident on the device, with sentinels in every
    row, pad column and output a call must leave alone.  `lean` drops every
    optional row: first_index, snap_index, lead_transferee, vote, cs_ids and
    half of the configuration rows."""

    def __init__(self, engine, nodes, R, S, stride=None, goff=0, lean=False):
        self.e, self.nodes, self.R, self.S, self.goff, self.lean = engine, nodes, R, S, goff, lean
        self.G = G = len(nodes)
        extras = ("self_slot",) if lean else ("self_slot", "lead_transferee", "snap_index")
        self.ps = ps = engine.ProgressState(G, S, 1, R, DEV, stride=stride, group_offset=goff,
                                            extras=extras)
        self.stride = ps.stride
        for k in QUIET:  # rows of the leader's half
            getattr(ps, k).random_()
        self.quiet = {k: getattr(ps, k).clone() for k in QUIET}
        a = sm.pack_snodes(nodes, R, S, self.stride, fill=SENT)
        ps.load_host(**{k: a[k] for k in LOG + ("run_first", "run_term")})
        if lean:
            ps.first_index = None
        self.fol = engine.Follower(ps, vote=not lean)
        self.fol.load_host(**{k: a[k] for k in FOL if getattr(self.fol, k) is not None})
        self.conf = cs = engine.ConfState(G, S, DEV)
        cs.slot_ids.copy_(torch.from_numpy(a["c_slot_ids"].view(np.int64)).to(DEV))
        for k in sm.CONF_MASKS:
            v = a["c_" + k]
            getattr(cs, k).copy_(torch.from_numpy(v.view(np.int16) if v.dtype == np.uint16 else v))
        cs.auto_leave.copy_(torch.from_numpy(a["c_auto_leave"]))
        if lean:
            cs.slot_ids = cs.learners_next = cs.is_learner = cs.auto_leave = None

    def host(self):
        ps, cs = self.ps, self.conf
        h = {k: (None if getattr(ps, k) is None else getattr(ps, k).cpu().numpy()) for k in LOG}
        for k in ("committed", "last_index", "first_index", "snap_index"):
            h[k] = None if h[k] is None else h[k].view(np.uint64)
        h["run_first"], h["run_term"] = u64(ps.run_first), u64(ps.run_term)
        h.update(self.fol.host())
        md = sm.mask_dtype(self.S)
        for k in sm.CONF_MASKS:
            t = getattr(cs, k)
            h["c_" + k] = None if t is None else t.cpu().numpy().view(md)
        h["c_auto_leave"] = None if cs.auto_leave is None else cs.auto_leave.cpu().numpy()
        h["c_slot_ids"] = None if cs.slot_ids is None else u64(cs.slot_ids)
        return h

    def compare(self, before, after_nodes, what):
        """The whole resident state against the model's nodes."""
        G, R = self.G, self.R
        got = self.host()
        want = sm.pack_snodes(after_nodes, R, self.S, self.stride)
        touched = np.array([a is not b for a, b in zip(after_nodes, self.nodes)])
        for k in LOG + FOL + CONF:
            if got[k] is None:
                continue
            g, w, b = got[k], want[k], before[k]
            if k == "c_slot_ids":
                g, w, b = (x.reshape(self.S, G) for x in (g, w, b))
                np.testing.assert_array_equal(g[:, ~touched], b[:, ~touched], err_msg=what + k)
            else:
                np.testing.assert_array_equal(g[~touched], b[~touched],
                                              err_msg=what + k + " of untouched groups")
            np.testing.assert_array_equal(g, w, err_msg=what + k)
        cnt = want["run_count"].astype(np.int64)
        live = np.arange(R)[:, None] < cnt[None, :]
        for k in ("run_first", "run_term"):
            g2, b2, w2 = (x[k].reshape(R, self.stride) for x in (got, before, want))
            np.testing.assert_array_equal(g2[:, :G][live], w2[:, :G][live], err_msg=what + k)
            # rows past the new count are not state: never written
            np.testing.assert_array_equal(g2[:, :G][~live], b2[:, :G][~live], err_msg=what + k)
            np.testing.assert_array_equal(g2[:, G:], b2[:, G:], err_msg=what + k + " pad")
            np.testing.assert_array_equal(g2[:, :G][:, ~touched], b2[:, :G][:, ~touched],
                                          err_msg=what + k + " of untouched groups")
        for k in QUIET:
            assert torch.equal(getattr(self.ps, k), self.quiet[k]), what + k
        self.nodes = after_nodes

    def stats_equal(self, st, stats, what):
        folded = self.e.stats_reduce(st).cpu().numpy().view(np.uint64)
        ws = np.zeros(16, np.uint64)
        for k, v in stats.items():
            ws[k] = v
        np.testing.assert_array_equal(folded, ws, err_msg=what + "stats")
        self.last_stats = folded

    def snap(self, msgs, with_stats=True):
        """One qe_snapshot_step, compared with the model; -> the model's outs."""
        e, ps = self.e, self.ps
        smg = e.SnapMsgs(ps, ids=not self.lean)
        smg.load_host(**sm.pack_smsgs(msgs, self.S, self.stride))
        out = e.SnapOut(ps)
        out.resp_index.fill_(SENT)
        out.result.fill_(S8)
        out.events.fill_(S8)
        st = e.stats_buffer(DEV) if with_stats else None
        before = self.host()
        assert e.snapshot_step(ps, self.fol, self.conf, smg, out, st) is out
        after, outs, stats = sm.step_batch(self.nodes, msgs, self.S, self.R, self.goff)
        o = out.host()
        np.testing.assert_array_equal(o["result"], [x["result"] for x in outs], err_msg="result")
        np.testing.assert_array_equal(o["events"], [x["events"] for x in outs], err_msg="events")
        np.testing.assert_array_equal(
            o["resp_index"], np.array([x.get("resp_index", SENT) for x in outs], np.uint64))
        self.compare(before, after, "snapshot_step: ")
        if with_stats:
            self.stats_equal(st, stats, "snapshot_step: ")
        return outs

    def compact(self, reqs, with_stats=True, create=True, applied=True):
        """One qe_compact with (ci, si, applied) per group; -> the model's outs."""
        e, ps = self.e, self.ps
        if not create:
            reqs = [(ci, 0, ap) for ci, _, ap in reqs]
        if not applied:
            reqs = [(ci, si, None) for ci, si, _ in reqs]
        cp = e.Compaction(ps, create=create, applied=applied)
        cp.load_host(compact_index=np.array([r[0] for r in reqs], np.uint64),
                     create_index=np.array([r[1] for r in reqs], np.uint64),
                     applied=np.array([r[2] or 0 for r in reqs], np.uint64))
        cp.result.fill_(S8)
        if create:
            cp.snap_term.fill_(SENT)
        st = e.stats_buffer(DEV) if with_stats else None
        before = self.host()
        assert e.compact(ps, cp, st) is cp
        after, outs, stats = sm.compact_batch(self.nodes, reqs, self.goff,
                                              have_snap=ps.snap_index is not None)
        o = cp.host()
        np.testing.assert_array_equal(o["result"], [x["result"] for x in outs], err_msg="result")
        if create:
            np.testing.assert_array_equal(
                o["snap_term"], np.array([x.get("snap_term", SENT) for x in outs], np.uint64))
        self.compare(before, after, "compact: ")
        if with_stats:
            self.stats_equal(st, stats, "compact: ")
        return outs


def neighbours(rng, G, R, S):
    nodes = [sm.gen_snode(rng, R, S) for _ in range(G)]
    return nodes, [sm.gen_smsg(rng, n, S) for n in nodes]


G4 = 197  # three tiles and a ragged fourth
SPOTS = (0, 63, 64, G4 - 1)


def test_fixture_rows_and_trace_deliveries_at_four_tile_positions(eng):
    rng = np.random.default_rng(47)
    cases = [(cid, sn, m, 4) for cid, sn, m in fixture_cases()]
    cases += [(c[0], c[1], c[2], 7) for c in trace_cases()]
    assert len(cases) == 7 * 2 + 2 + 1 + 7
    for cid, sn, m, s_case in cases:
        S, R = 7, 8
        nodes, msgs = neighbours(rng, G4, R, S)
        # the case in the batch's slot count: its masks and ids padded to S
        conf = sm.Conf(S, *[getattr(sn.conf, k) for k in sm.CONF_MASKS],
                       auto_leave=sn.conf.auto_leave,
                       ids=list(sn.conf.ids) + [0] * (S - len(sn.conf.ids)))
        node = sm.SNode(sn.node, conf, sn.self_slot, sn.snap_index)
        msg = sm.SMsg(m.type, m.frm, m.term, m.sindex, m.sterm, m.inc, m.out, m.learner,
                      m.learners_next, m.auto_leave, ids=[s + 1 for s in range(S)])
        want_after, want_out = sm.step(sn, m, s_case)
        for pos in SPOTS:
            nodes[pos], msgs[pos] = node, msg
        h = Harness(eng, nodes, R, S)
        outs = h.snap(msgs)
        for pos in SPOTS:  # the same answer as in the case's own slot count (checked on the CPU)
            assert outs[pos] == want_out, cid
            assert h.nodes[pos].conf.string() == want_after.conf.string(), cid


def test_compaction_tables_at_four_tile_positions(eng):
    """TestStorageCompact, TestStorageCreateSnapshot and TestCompaction (one
    run of 1000 entries) among random neighbours.  TestCompactionSideEffects
    needs 1000 runs: it is the CPU model's alone."""
    from tests.test_snapshot_model import tables
    rng = np.random.default_rng(53)
    t = tables()
    seqs = []
    for row in t["TestStorageCompact"]["rows"]:
        seqs.append((storage(t["TestStorageCompact"]["ents"]), [(row["i"], 0)]))
    for row in t["TestStorageCreateSnapshot"]["rows"]:
        seqs.append((storage(t["TestStorageCreateSnapshot"]["ents"]), [(0, row["i"]), (0, row["i"])]))
    for _, sn, seq, _ in compaction_cases():
        seqs.append((sn, [(ci, 0) for ci, _ in seq]))
    R, S = 4, 3
    for sn, seq in seqs:
        nodes = [sm.gen_snode(rng, R, S) for _ in range(G4)]
        for pos in SPOTS:
            nodes[pos] = sn
        h = Harness(eng, nodes, R, S)
        for ci, si in seq:
            reqs = [sm.gen_compaction(rng, n) for n in h.nodes]
            for pos in SPOTS:
                reqs[pos] = (ci, si, h.nodes[pos].node.committed)
            outs = h.compact(reqs)
            assert len({repr(sorted(outs[p].items())) for p in SPOTS}) == 1


@pytest.mark.parametrize("S,R,lean", [(3, 4, False), (8, 5, True), (9, 8, False), (16, 16, False),
                                      (16, 4, True)])
def test_random_differential(eng, S, R, lean):
    """Both mask widths at their edges, the run buckets at theirs, a stride
    that is no multiple of anything, a group offset, optional rows NULL, and
    consecutive calls on the same rows: compact, restore, compact again."""
    rng = np.random.default_rng(9000 + 17 * S + R)
    G = 64 * 9 + 21
    nodes = [sm.gen_snode(rng, R, S) for _ in range(G)]
    h = Harness(eng, nodes, R, S, stride=G + 11, goff=1 << 33, lean=lean)
    seen_s, seen_c = set(), set()
    for rnd in range(3):
        outs = h.compact([sm.gen_compaction(rng, n) for n in h.nodes], create=not lean,
                         applied=not (lean and rnd == 1))
        seen_c |= {o["result"] for o in outs}
        seen_s |= {o["result"] for o in h.snap([sm.gen_smsg(rng, n, S) for n in h.nodes])}
    outs = h.compact([sm.gen_compaction(rng, n) for n in h.nodes], with_stats=False,
                     create=not lean)
    assert seen_s == set(sm.SR_NAMES), sorted(set(sm.SR_NAMES) - seen_s)
    want_c = {sm.CP_NONE, sm.CP_COMPACTED, sm.CP_ALREADY, sm.CP_OUT_OF_BOUND, sm.CP_PAST_APPLIED}
    if not lean:
        want_c |= {sm.CP_CREATED, sm.CP_CREATED | sm.CP_COMPACTED, sm.CP_SNAP_OUT_OF_DATE}
    assert want_c <= seen_c, sorted(want_c - seen_c)


@pytest.mark.parametrize("case", lift.SNAP_CASES, ids=str)
def test_wide_differential(eng, case):
    """Four rounds of qe_snapshot_step then qe_compact on one state whose
    indexes and terms are lifted per group (tests/lift.py; `applied` with
    them): both mask widths, the three run buckets, nine tiles and a ragged
    one, statistics on, the model on the wide values.  Per index base every
    answer of a MsgSnap and of a compaction is met (on the CPU in
    tests/test_lift_model.py, and asserted here on what the device went
    through)."""
    S, R = case
    box = {}

    def harness(nodes):
        if not box:
            box["h"] = Harness(eng, nodes, R, S, stride=lift.G + lift.PAD, goff=lift.GOFF)
        return box["h"]

    def snapper(nodes, msgs):
        outs = harness(nodes).snap(msgs)
        return box["h"].nodes, outs

    def compacter(nodes, reqs):
        outs = harness(nodes).compact(reqs)
        return box["h"].nodes, outs

    ls, slog, clog = lift.snap_run(case, snapper, compacter)
    lift.check_snap_coverage(ls, slog, clog)


def test_top_of_range(eng):
    """2^64 - 1 is QE_INDEX_INF and no log index: a MsgSnap there is
    QE_SR_BAD_MSG, one at 2^64 - 2 restores with first_index = 2^64 - 1, a
    compaction at a last index of 2^64 - 2 leaves first_index = 2^64 - 1 and
    one at 2^64 - 1 is out of bound.  Each row of lift.snap_top_rows() at lane
    0, 63, 64 and the last lane of a partial tile among random lifted
    neighbours; the rows' literals hold the model."""
    rng = np.random.default_rng(89)
    R, S = 8, 3
    for row in lift.snap_top_rows(S):
        _, sn, msg, req, _ = row
        nodes, msgs, reqs = lift.snap_neighbours(rng, G4, R, S)
        for pos in SPOTS:
            nodes[pos] = sn
            if msg is not None:
                msgs[pos] = msg
            else:
                reqs[pos] = req
        h = Harness(eng, nodes, R, S, stride=G4 + 5, goff=1 << 33)
        outs = h.snap(msgs) if msg is not None else h.compact(reqs)
        for pos in SPOTS:
            lift.check_snap_top_row(row, h.nodes[pos], outs[pos])
        assert len({repr(sorted(outs[p].items())) for p in SPOTS}) == 1, row[0]


def test_one_snapshot_in_a_sea_of_none(eng):
    """A sparse batch: no byte of any other group moves (Harness.compare), the
    statistics count one group, and an all-NONE batch counts none."""
    rng = np.random.default_rng(59)
    G, R, S = 64 * 5 + 9, 4, 5
    nodes = [sm.gen_snode(rng, R, S) for _ in range(G)]
    h = Harness(eng, nodes, R, S, stride=G + 3)
    outs = h.snap([sm.SMsg() for _ in range(G)])
    assert all(o == {"result": sm.SR_NONE, "events": 0} for o in outs)
    assert not h.last_stats.any()
    outs = h.compact([(0, 0, 0)] * G)
    assert all(o == {"result": sm.CP_NONE} for o in outs) and not h.last_stats.any()
    msgs = [sm.SMsg() for _ in range(G)]
    g = 64 * 2 + 5
    n = h.nodes[g]
    msgs[g] = sm.SMsg(sm.SMSG_SNAP, 1, n.node.term + 1, n.node.last_index() + 7, n.node.term + 1,
                      inc=(1 << S) - 1, ids=[s + 1 for s in range(S)])
    n.self_slot = 2
    h = Harness(eng, h.nodes, R, S, stride=G + 3)
    outs = h.snap(msgs)
    assert outs[g]["result"] == sm.SR_RESTORED and h.last_stats[sm.STAT_GROUPS] == 1
    assert [i for i, o in enumerate(outs) if o["result"]] == [g]
    h.snap(msgs, with_stats=False)  # the same message again: stale now


def test_lower_term_is_ignored_whatever_the_flags(eng):
    """The preamble's one difference from qe_follower_step."""
    G, S = 70, 3
    nodes = [sm.SNode(fm.Node([(0, 0)], term=5, lead=1), sm.Conf(S, 7, ids=[1, 2, 3]), 0, 0)
             for _ in range(G)]
    h = Harness(eng, nodes, 4, S)
    h.fol.flags = _lib.QE_FOLLOW_CHECK_QUORUM | _lib.QE_FOLLOW_PREVOTE
    outs = h.snap([sm.SMsg(sm.SMSG_SNAP, 1, 4, 9, 4, 7) for _ in range(G)])
    assert all(o == {"result": sm.SR_IGNORED, "events": 0} for o in outs)


def test_einval_table(eng):
    G, S, R = 10, 3, 4
    h = Harness(eng, [sm.gen_snode(np.random.default_rng(1), R, S) for _ in range(G)], R, S)
    ps, L = h.ps, _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)

    def snap(edit=None, null=None):
        p, f, c = ps.struct(), h.fol.struct(), h.conf.struct()
        m, o = eng.SnapMsgs(ps, ids=True), eng.SnapOut(ps)
        keep = (m, o)  # noqa: F841
        ms, os_ = m.struct(), o.struct()
        if edit:
            edit(p, f, c, ms, os_)
        args = [C.byref(p), C.byref(f), C.byref(c), C.byref(ms), C.byref(os_)]
        if null is not None:
            args[null] = None
        return L.qe_snapshot_step(*args, None, stream)

    def compact(edit=None, null=None):
        p = ps.struct()
        cp = eng.Compaction(ps)
        c = cp.struct()
        if edit:
            edit(p, c)
        args = [C.byref(p), C.byref(c)]
        if null is not None:
            args[null] = None
        return L.qe_compact(*args, None, stream)

    def setter(i, name, value=None):
        def edit(*structs):
            setattr(structs[i], name, value)
        return edit

    assert snap() == _lib.QE_OK and compact() == _lib.QE_OK
    for k in range(5):
        assert snap(null=k) == _lib.QE_EINVAL, k
    for k in range(2):
        assert compact(null=k) == _lib.QE_EINVAL, k
    bad_snap = [(0, n) for n in ("committed", "last_index", "run_first", "run_term", "run_count",
                                 "self_slot")]
    bad_snap += [(1, n) for n in ("term", "state", "lead")]
    bad_snap += [(3, n) for n in ("type", "from_", "term", "snap_index", "snap_term", "cs_inc",
                                  "cs_out", "cs_learner", "cs_learners_next", "cs_auto_leave")]
    bad_snap += [(4, "result")]
    for i, n in bad_snap:
        assert snap(setter(i, n)) == _lib.QE_EINVAL, n
    for i, n, v in ((2, "num_groups", G + 1), (2, "num_slots", S + 1), (2, "reserved", 1),
                    (0, "stride", G - 1), (0, "log_runs", 0), (0, "log_runs", 17),
                    (0, "num_slots", 17)):
        assert snap(setter(i, n, v)) == _lib.QE_EINVAL, n
    for n in ("committed", "last_index", "run_first", "run_term", "run_count"):
        assert compact(setter(0, n)) == _lib.QE_EINVAL, n
    for n in ("compact_index", "result"):
        assert compact(setter(1, n)) == _lib.QE_EINVAL, n
    assert compact(setter(0, "snap_index")) == _lib.QE_EINVAL  # create_index without it
    for n, v in (("stride", G - 1), ("log_runs", 0), ("log_runs", 17)):
        assert compact(setter(0, n, v)) == _lib.QE_EINVAL, n
    # optional rows and an empty batch
    assert snap(setter(3, "cs_ids")) == _lib.QE_OK and snap(setter(4, "events")) == _lib.QE_OK
    assert compact(setter(1, "applied")) == _lib.QE_OK

    def empty(p, *rest):
        p.num_groups = 0
        if len(rest) == 4:
            rest[1].num_groups = 0
    assert snap(empty) == _lib.QE_OK and compact(empty) == _lib.QE_OK
    torch.cuda.synchronize()


def test_closed_loop_slow_node_restore(eng):
    """TestSlowNodeRestore / snapshot_succeed_via_app_resp on the device,
    clusters of three: qe_compact on the leader, qe_progress_send reports the
    MsgSnap for the lagging peer, qe_snapshot_step on that peer, its resp_index
    goes in as MsgAppResp to qe_progress_step (Snapshot -> Probe -> Replicate
    and the next MsgApp), qe_follower_step catches the peer up; the committed
    indices converge and equal the models'."""
    e = eng
    rng = np.random.default_rng(61)
    G, S, R, F = 64 * 2 + 11, 3, 4, 4
    L = rng.integers(4, 40, G).astype(np.uint64)       # the leader's last index, all committed
    ci = np.array([int(rng.integers(1, int(x))) for x in L], np.uint64)  # compacted and snapshotted at
    lead = e.ProgressState(G, S, F, R, DEV, extras=("self_slot", "snap_index", "tracked"))
    st = lead.stride
    row = lambda v: np.array(v, np.uint64)  # noqa: E731
    match = np.zeros(S * st, np.uint64)
    nxt = np.ones(S * st, np.uint64)
    flags = np.zeros(S * st, np.uint8)
    for s in (0, 1):
        match[s * st: s * st + G] = L
        nxt[s * st: s * st + G] = L + 1
        flags[s * st: s * st + G] = _lib.QE_PR_REPLICATE | _lib.QE_PF_RECENT_ACTIVE
    flags[2 * st: 2 * st + G] = _lib.QE_PR_PROBE | _lib.QE_PF_RECENT_ACTIVE
    run_first, run_term = np.zeros(R * st, np.uint64), np.zeros(R * st, np.uint64)
    run_first[st: st + G] = 1
    run_term[st: st + G] = 1
    lead.load_host(match=match, next=nxt, flags=flags, committed=row(L), last_index=row(L),
                   term_start=np.ones(G, np.uint64), first_index=np.ones(G, np.uint64),
                   run_first=run_first, run_term=run_term, run_count=np.full(G, 2, np.uint8),
                   self_slot=np.zeros(G, np.uint8), snap_index=np.zeros(G, np.uint64),
                   tracked=np.full(G, 7, np.uint8))
    # 1. the leader compacts its log and keeps a snapshot at the same index
    cp = e.Compaction(lead)
    cp.load_host(compact_index=ci, create_index=ci, applied=row(L))
    e.compact(lead, cp)
    assert (cp.result.cpu().numpy() == sm.CP_CREATED | sm.CP_COMPACTED).all()
    np.testing.assert_array_equal(u64(lead.first_index), ci + 1)
    np.testing.assert_array_equal(u64(cp.snap_term), np.ones(G, np.uint64))
    # 2. its next send to the lagging peer is a MsgSnap (Next 1 < firstIndex)
    want = torch.full((G,), 4, dtype=torch.uint8, device=DEV)
    sent, snap = e.progress_send(lead, want, send_if_empty=True)
    assert (snap.cpu().numpy() == 4).all()
    hl = lead.host()
    assert ((hl["flags"].reshape(S, st)[2, :G] & _lib.QE_PF_STATE) == _lib.QE_PR_SNAPSHOT).all()
    np.testing.assert_array_equal(hl["pending"].reshape(S, st)[2, :G], ci)
    # 3. the peer (slot 2): an empty log at term 0, restored by qe_snapshot_step
    nodes = [sm.SNode(fm.Node([(0, 0)]), sm.Conf(S), 2, 0) for _ in range(G)]
    h = Harness(eng, nodes, R, S)
    smg = e.SnapMsgs(h.ps, ids=True)
    smg.type.fill_(sm.SMSG_SNAP)
    smg.term.fill_(1)
    smg.snap_index.copy_(lead.snap_index)     # device to device: nothing is rewritten by hand
    smg.snap_term.copy_(cp.snap_term)
    smg.cs_inc.fill_(7)
    smg.load_host(cs_ids=sm.pack_smsgs([sm.SMsg()] * G, S, h.stride)["cs_ids"])
    out = e.snapshot_step(h.ps, h.fol, h.conf, smg)
    msgs = [sm.SMsg(sm.SMSG_SNAP, 0, 1, int(c), 1, 7, ids=[1, 2, 3]) for c in ci]
    after, outs, _ = sm.step_batch(h.nodes, msgs, S, R)
    o = out.host()
    assert (o["result"] == sm.SR_RESTORED).all() and (o["events"] == fm.TEV_RESET).all()
    np.testing.assert_array_equal(o["resp_index"], ci)
    np.testing.assert_array_equal(u64(h.ps.committed), [n.node.committed for n in after])
    assert (h.conf.inc.cpu().numpy() == 7).all() and (h.conf.tracked.cpu().numpy() == 7).all()
    # 4. resp_index goes in as the MsgAppResp of slot 2
    pm = e.PeerMsgs(lead)
    pm.type[2 * st: 2 * st + G].fill_(_lib.QE_MSG_APP_RESP)
    pm.index[2 * st: 2 * st + G].copy_(out.resp_index)
    e.progress_step(lead, pm)
    hl = lead.host()
    assert ((hl["flags"].reshape(S, st)[2, :G] & _lib.QE_PF_STATE) == _lib.QE_PR_REPLICATE).all()
    np.testing.assert_array_equal(hl["match"].reshape(S, st)[2, :G], ci)
    np.testing.assert_array_equal(hl["next"].reshape(S, st)[2, :G], L + 1)
    assert not hl["pending"].reshape(S, st)[2, :G].any()
    assert (pm.msg_count.cpu().numpy().reshape(S, st)[2, :G] == 1).all()
    np.testing.assert_array_equal(u64(pm.msg_index).reshape(S, st)[2, :G], ci)
    # 5. the MsgApp that follows, built from the leader's rows, catches the peer up
    lm = e.LeaderMsgs(h.ps, 1)
    lm.type.fill_(fm.LMSG_APP)
    lm.term.fill_(1)
    lm.index.copy_(pm.msg_index[2 * st: 2 * st + G])
    lm.log_term.copy_(cp.snap_term)
    lm.commit.copy_(lead.committed)
    lm.ent_len[:G].copy_((lead.last_index - lm.index).to(torch.int32))
    lm.ent_term[:G].fill_(1)
    fo = e.follower_step(h.ps, h.fol, lm)
    final = [fm.step(n.node, fm.Msg(fm.LMSG_APP, 0, 1, int(c), 1, int(x), [(int(x - c), 1)]),
                     0, S, R) for n, c, x in zip(after, ci, L)]
    assert (fo.result.cpu().numpy() == fm.FR_APP_ACCEPT).all()
    assert all(o_["result"] == fm.FR_APP_ACCEPT for _, o_ in final)
    np.testing.assert_array_equal(u64(fo.resp_index), L)
    for k in ("committed", "last_index"):
        np.testing.assert_array_equal(u64(getattr(h.ps, k)), u64(getattr(lead, k)), err_msg=k)
    np.testing.assert_array_equal(u64(h.ps.committed), [n.committed for n, _ in final])
    np.testing.assert_array_equal(h.ps.run_count.cpu().numpy(), [len(n.runs) for n, _ in final])


def test_runs_full_then_compact_then_accept(eng):
    """A filled run table refuses the next term's entry (QE_FR_RUNS_FULL);
    qe_compact frees rows on the device; the same MsgApp is accepted."""
    e = eng
    G, S, R = 64 + 13, 3, 4
    ents = [(0, 0), (1, 1), (2, 2), (3, 3)]
    nodes = [sm.SNode(fm.Node(ents, committed=3, term=3, lead=0), sm.Conf(S, 7, ids=[1, 2, 3]), 1, 0)
             for _ in range(G)]
    h = Harness(eng, nodes, R, S)
    m = fm.Msg(fm.LMSG_APP, 0, 4, 3, 3, 3, [(1, 4)])
    lm = e.LeaderMsgs(h.ps, 1)
    lm.load_host(**fm.pack_msgs([m] * G, 1, h.stride))
    assert (e.follower_step(h.ps, h.fol, lm).result.cpu().numpy() == fm.FR_RUNS_FULL).all()
    assert fm.step(nodes[0].node, m, 0, S, R)[1]["result"] == fm.FR_RUNS_FULL
    outs = h.compact([(3, 0, 3)] * G)
    assert all(o["result"] == sm.CP_COMPACTED and o["rstar"] == 3 for o in outs)
    fo = e.follower_step(h.ps, h.fol, lm)
    after, out = fm.step(h.nodes[0].node, m, 0, S, R)
    assert out["result"] == fm.FR_APP_ACCEPT and after.runs == [(3, 3), (4, 4)]
    assert (fo.result.cpu().numpy() == fm.FR_APP_ACCEPT).all()
    np.testing.assert_array_equal(h.ps.run_count.cpu().numpy(), np.full(G, 2))
    rf = u64(h.ps.run_first).reshape(R, h.stride)
    rt = u64(h.ps.run_term).reshape(R, h.stride)
    assert (rf[0, :G] == 3).all() and (rt[0, :G] == 3).all()
    assert (rf[1, :G] == 4).all() and (rt[1, :G] == 4).all()
    np.testing.assert_array_equal(u64(h.ps.last_index), np.full(G, 4, np.uint64))


def walk_state(eng, base_nodes):
    """The base's SNodes repeated (tests/walk.py) and resident -> (ps, fol,
    conf, G, stride)."""
    from tests import walk
    R, S = walk.R, walk.S
    G = walk.walk_groups(torch.cuda.get_device_properties(DEV).multi_processor_count)
    stride = G + walk.PAD
    a = walk.repeat(sm.pack_snodes(base_nodes, R, S, walk.PERIOD), G, stride, walk_rows(G),
                    fill=SENT)
    ps = eng.ProgressState(G, S, 1, R, DEV, stride=stride, group_offset=walk.GOFF,
                           extras=("self_slot", "lead_transferee", "snap_index"))
    ps.load_host(**{k: a[k] for k in LOG + ("run_first", "run_term")})
    fol = eng.Follower(ps)
    fol.load_host(**{k: a[k] for k in FOL})
    cs = eng.ConfState(G, S, DEV)
    cs.slot_ids.copy_(torch.from_numpy(a["c_slot_ids"].view(np.int64)).to(DEV))
    for k in sm.CONF_MASKS:
        getattr(cs, k).copy_(torch.from_numpy(a["c_" + k]))
    cs.auto_leave.copy_(torch.from_numpy(a["c_auto_leave"]))
    return ps, fol, cs, G, stride


def walk_rows(G):
    from tests import walk
    return {"run_first": walk.R, "run_term": walk.R, "c_slot_ids": (walk.S, G)}


def walk_compare(ps, fol, cs, G, stride, after_nodes):
    """The resident state against the base's nodes after the call, repeated;
    -> the expectation."""
    from tests import walk
    R, S = walk.R, walk.S
    want = walk.repeat(sm.pack_snodes(after_nodes, R, S, walk.PERIOD), G, stride, walk_rows(G),
                       fill=SENT)
    got = {k: getattr(ps, k).cpu().numpy() for k in LOG}
    for k in ("committed", "last_index", "first_index", "snap_index"):
        got[k] = got[k].view(np.uint64)
    got.update(fol.host())
    for k in sm.CONF_MASKS:
        got["c_" + k] = getattr(cs, k).cpu().numpy()
    got["c_auto_leave"], got["c_slot_ids"] = cs.auto_leave.cpu().numpy(), u64(cs.slot_ids)
    for k in LOG + FOL + CONF:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    live = np.arange(R)[:, None] < want["run_count"].astype(np.int64)[None, :]
    for k in ("run_first", "run_term"):
        g2, w2 = u64(getattr(ps, k)).reshape(R, stride), want[k].reshape(R, stride)
        np.testing.assert_array_equal(g2[:, :G][live], w2[:, :G][live], err_msg=k)
        np.testing.assert_array_equal(g2[:, G:], w2[:, G:], err_msg=k + " pad")
    return want


def test_snapshot_walking_waves(eng):
    """One qe_snapshot_step in which every wave walks two or three tiles
    (tests/walk.py): the base's 209 groups repeated, statistics on, a group
    offset past 2^32 and a stride that is no multiple of 64.  Every row is the
    base's expectation repeated, every counter the repeated base's sum."""
    from tests import walk
    b = walk.snap_base()
    ps, fol, cs, G, stride = walk_state(eng, b.nodes)
    idx = np.arange(G) % walk.PERIOD
    smg = eng.SnapMsgs(ps, ids=True)
    smg.load_host(**walk.repeat(sm.pack_smsgs(b.msgs, walk.S, walk.PERIOD), G, stride,
                                {"cs_ids": walk.S}))
    out = eng.SnapOut(ps)
    out.resp_index.fill_(SENT)
    out.result.fill_(S8)
    out.events.fill_(S8)
    st = eng.stats_buffer(DEV)
    eng.snapshot_step(ps, fol, cs, smg, out, st)
    want = walk_compare(ps, fol, cs, G, stride, b.after)
    o = out.host()
    res = np.array([x["result"] for x in b.outs], np.uint8)[idx]
    np.testing.assert_array_equal(o["result"], res, err_msg="result")
    np.testing.assert_array_equal(o["events"], np.array([x["events"] for x in b.outs])[idx])
    np.testing.assert_array_equal(
        o["resp_index"], np.array([x.get("resp_index", SENT) for x in b.outs], np.uint64)[idx])
    folded = eng.stats_reduce(st).cpu().numpy().view(np.uint64)
    ws = walk.expect_stats(b.shares, G, walk.snap_hashes(want, res))
    np.testing.assert_array_equal(folded, ws, err_msg="stats")
    assert ws[sm.STAT_GROUPS] > 0.6 * G and ws[sm.STAT_GRANTED] and ws[sm.STAT_COMMIT_ADVANCED]


def test_compact_walking_waves(eng):
    """The same shape through qe_compact."""
    from tests import walk
    b = walk.compact_base()
    ps, fol, cs, G, stride = walk_state(eng, b.nodes)
    idx = np.arange(G) % walk.PERIOD
    cp = eng.Compaction(ps)
    cp.load_host(compact_index=np.array([r[0] for r in b.reqs], np.uint64)[idx],
                 create_index=np.array([r[1] for r in b.reqs], np.uint64)[idx],
                 applied=np.array([r[2] for r in b.reqs], np.uint64)[idx])
    cp.result.fill_(S8)
    cp.snap_term.fill_(SENT)
    st = eng.stats_buffer(DEV)
    eng.compact(ps, cp, st)
    want = walk_compare(ps, fol, cs, G, stride, b.after)
    o = cp.host()
    res = np.array([x["result"] for x in b.outs], np.uint8)[idx]
    np.testing.assert_array_equal(o["result"], res, err_msg="result")
    np.testing.assert_array_equal(
        o["snap_term"], np.array([x.get("snap_term", SENT) for x in b.outs], np.uint64)[idx])
    folded = eng.stats_reduce(st).cpu().numpy().view(np.uint64)
    ws = walk.expect_stats(b.shares, G, walk.compact_hashes(want, res))
    np.testing.assert_array_equal(folded, ws, err_msg="stats")
    assert ws[sm.STAT_GROUPS] > 0.6 * G and ws[sm.STAT_COMPACTED]
