"""A lift of the receiver-side models' states and messages to wide values.

The generators of tests/follower_model.py, vote_model.py and snapshot_model.py
draw indexes below about 100 and terms below about 30, so the high dword of
every word the step kernels load or store is 0.  The lift turns a small state
or message into a wide one and back; the generators stay as they are, so their
random streams do not change.

  index      i -> i + B, clamped at 2^64 - 1 (a message the generator put at
             the top of the range stays there);
  term       t -> t + T for t > 0, 0 stays 0: entry terms, LogTerm, the terms
             of a message's runs, the snapshot's term, and the Term of an
             election message, where 0 marks a local message or a bad one;
  own term   t -> t + T always: the node's Term (a campaign from term 0 gives
             T + 1, which lowers to 1) and the Term of a MsgApp, MsgHeartbeat
             or MsgSnap, which is its sender's own Term and is compared with
             the receiver's as it is.
  counts, slots, masks, flags and types are not touched; a compaction or
  create index of 0 is "no request" and stays 0.

Both maps preserve order within their class, so a model step commutes with the
lift wherever no index is clamped (tests/test_lift_model.py).

One pair (B, T) per group, cycling so that every B meets every T.  2^32 - k
makes indexes and terms cross the dword boundary inside one group's log,
2^63 - k the sign bit of the int64 tensors, 2^64 - 4096 stays clear of the
wrap (term wrap at 2^64 - 1 is out of scope).

A run of consecutive calls lowers the evolving wide state, draws the messages
with the model's own generator on the small state, and lifts them.  The runs
below are the ones tests/test_gpu_follower.py, test_gpu_vote.py and
test_gpu_snapshot.py make on the device; tests/test_lift_model.py proves on
the model alone that each meets its coverage conditions."""
import numpy as np

from tests import follower_model as fm
from tests import snapshot_model as sm
from tests import vote_model as vm

M64 = fm.M64
IB = (0, (1 << 32) - 9, (1 << 32) - 40, (1 << 53) + 1, (1 << 63) - 17, M64 - 4095)
TB = (0, (1 << 32) - 2, (1 << 32) - 5, (1 << 63) - 3, M64 - 4095)
G, PAD, GOFF = 601, 11, 1 << 33  # nine tiles and a ragged one of 25 lanes


class Lift:
    def __init__(self, B, T, down=False):
        self.B, self.T, self.down = B, T, down

    def inv(self):
        return Lift(self.B, self.T, not self.down)

    def i(self, i):
        if self.down:
            assert i >= self.B, (i, self.B)
            return i - self.B
        return min(i + self.B, M64)

    def t(self, t):
        if not t:
            return 0
        if self.down:
            assert t > self.T, (t, self.T)
            return t - self.T
        return t + self.T

    def own(self, t):
        if self.down:
            assert t >= self.T, (t, self.T)
            return t - self.T
        return t + self.T

    def ents(self, ents):
        return [(self.i(i), self.t(t)) for i, t in ents]


def pair(g):
    return IB[g % len(IB)], TB[(g // len(IB)) % len(TB)]


def lifts(n):
    return [Lift(*pair(g)) for g in range(n)]


# ---- follower ----
def follower_node(n, L):
    return fm.Node(L.ents(n.ents), L.i(n.committed), L.own(n.term), n.state, n.lead, n.vote,
                   n.transferee, runs=L.ents(n.runs))


def follower_msg(m, L):
    if m.type == fm.LMSG_NONE:
        return fm.Msg()
    return fm.Msg(m.type, m.frm, L.own(m.term), L.i(m.index), L.t(m.log_term), L.i(m.commit),
                  [(n, L.t(t)) for n, t in m.runs])


def follower_out(o, L):
    """The outputs of a wide step, lowered (L = the group's lift, inverted)."""
    o = dict(o)
    if o["result"] in (fm.FR_APP_ACCEPT, fm.FR_APP_REJECT, fm.FR_APP_STALE):
        o["resp_index"] = L.i(o["resp_index"])
    if o.get("append_from"):
        o["append_from"] = L.i(o["append_from"])
    if "reject_hint" in o:
        o["reject_hint"], o["resp_log_term"] = L.i(o["reject_hint"]), L.t(o["resp_log_term"])
    return o


# ---- vote ----
def vote_node(n, L):
    return vm.Node(L.ents(n.ents), voted=n.voted, granted=n.granted, elapsed=n.elapsed, inc=n.inc,
                   out=n.out, tracked=n.tracked, self_slot=n.self_slot, no_campaign=n.no_campaign,
                   committed=L.i(n.committed), term=L.own(n.term), state=n.state, lead=n.lead,
                   vote=n.vote, transferee=n.transferee, runs=L.ents(n.runs))


def vote_msg(m, L):
    if m.type == vm.VMSG_NONE:
        return vm.Msg()
    return vm.Msg(m.type, m.frm, L.t(m.term), L.i(m.index), L.t(m.log_term), m.flags)


def vote_out(o, L):
    o = dict(o)
    if "resp_term" in o:
        o["resp_term"] = L.own(o["resp_term"])
    if "req_log_term" in o:
        o["req_log_term"] = L.t(o["req_log_term"])
    return o


# ---- snapshot / compact ----
def snap_node(sn, L):
    new = sm.SNode(follower_node(sn.node, L), sn.conf, sn.self_slot, L.i(sn.snap_index))
    new.first_index = L.i(sn.first_index)
    return new


def snap_msg(m, L):
    if m.type == sm.SMSG_NONE:
        return sm.SMsg()
    return sm.SMsg(m.type, m.frm, L.own(m.term), L.i(m.sindex), L.t(m.sterm), m.inc, m.out,
                   m.learner, m.learners_next, m.auto_leave, m.ids)


def snap_out(o, L):
    o = dict(o)
    if "resp_index" in o:
        o["resp_index"] = L.i(o["resp_index"])
    return o


def compaction(req, L):
    ci, si, ap = req
    return (L.i(ci) if ci else 0, L.i(si) if si else 0, None if ap is None else L.i(ap))


def compact_out(o, L):
    o = dict(o)
    if "snap_term" in o:
        o["snap_term"] = L.t(o["snap_term"])
    return o


# ---------------------------------------------------------------------------
# The lifted runs of the GPU differentials.  stepper(nodes, msgs) -> (nodes
# after, outs) replaces the model's own batch step (the device harness); each
# run returns (the lifts, the outs of every call).
# ---------------------------------------------------------------------------
FOLLOWER_CASES = [(1, 1, 3), (4, 4, 1), (16, 4, 0), (8, 0, 2)]  # (R, E, flags)
FOLLOWER_S = 5
SNAP_CASES = [(3, 4), (9, 8), (16, 16)]                         # (S, R)


def follower_run(case, stepper=None, calls=8, groups=G):
    R, E, flags = case
    S = FOLLOWER_S
    rng = np.random.default_rng(7101 + 31 * R + E)
    ls = lifts(groups)
    nodes = [follower_node(fm.gen_node(rng, R, S), L) for L in ls]
    log = []
    for _ in range(calls):
        small = [follower_node(n, L.inv()) for n, L in zip(nodes, ls)]
        msgs = [follower_msg(fm.gen_msg(rng, n, E, S), L) for n, L in zip(small, ls)]
        if stepper:
            nodes, outs = stepper(nodes, msgs)
        else:
            nodes, outs, _ = fm.step_batch(nodes, msgs, flags, S, R, GOFF)
        log.append(outs)
    return ls, log


def vote_run(case, stepper=None, calls=8, groups=G):
    S, R, masks, flags, cand, have_self = case
    rng = np.random.default_rng(9100 + 101 * S + 7 * R + flags + 2 * cand + have_self)
    ls = lifts(groups)
    nodes = [vote_node(vm.gen_node(rng, R, S, masks), L) for L in ls]
    log = []
    for _ in range(calls):
        small = [vote_node(n, L.inv()) for n, L in zip(nodes, ls)]
        msgs = [vote_msg(vm.gen_msg(rng, n, S), L) for n, L in zip(small, ls)]
        if stepper:
            nodes, outs = stepper(nodes, msgs)
        else:
            nodes, outs, _ = vm.step_batch(nodes, msgs, flags, S, 10, cand, have_self, GOFF)
        log.append(outs)
    return ls, log


def snap_run(case, snapper=None, compacter=None, rounds=4, groups=G):
    """-> (the lifts, the outs of every qe_snapshot_step, those of every qe_compact)."""
    S, R = case
    rng = np.random.default_rng(8100 + S)
    ls = lifts(groups)
    nodes = [snap_node(sm.gen_snode(rng, R, S), L) for L in ls]
    slog, clog = [], []
    for _ in range(rounds):
        small = [snap_node(n, L.inv()) for n, L in zip(nodes, ls)]
        msgs = [snap_msg(sm.gen_smsg(rng, n, S), L) for n, L in zip(small, ls)]
        if snapper:
            nodes, outs = snapper(nodes, msgs)
        else:
            nodes, outs, _ = sm.step_batch(nodes, msgs, S, R, GOFF)
        slog.append(outs)
        small = [snap_node(n, L.inv()) for n, L in zip(nodes, ls)]
        reqs = [compaction(sm.gen_compaction(rng, n), L) for n, L in zip(small, ls)]
        if compacter:
            nodes, outs = compacter(nodes, reqs)
        else:
            nodes, outs, _ = sm.compact_batch(nodes, reqs, GOFF)
        clog.append(outs)
    return ls, slog, clog


# ---------------------------------------------------------------------------
# The top of the range: 2^64 - 1 is QE_INDEX_INF, no log index.  Hand-built
# rows (M = 2^64 - 1; a log "ending at x" has its dummy entry at x - 3 and
# three entries, all of term 5); `want` restates the expectation as literals
# where the model is not to be the only witness, else it is None.
# ---------------------------------------------------------------------------
def log_ending_at(last, committed=None, term=5):
    ents = [(last - 3 + k, 5) for k in range(4)]
    return fm.Node(ents, committed=ents[0][0] if committed is None else committed, term=term, lead=1)


def follower_top_rows():
    """-> [(id, node, msg, want)]; want = (out, last_index, committed, last run) or None."""
    M, APP, HB = M64, fm.LMSG_APP, fm.LMSG_HEARTBEAT
    refused = lambda code: {"result": code, "events": 0}  # noqa: E731
    rows = [
        ("append reaching M", log_ending_at(M - 1), fm.Msg(APP, 1, 5, M - 1, 5, M, [(1, 5)]),
         (refused(fm.FR_BAD_MSG), M - 1, M - 4, (M - 4, 5))),
        ("the highest legal append", log_ending_at(M - 2),
         fm.Msg(APP, 1, 5, M - 2, 5, M - 1, [(1, 5)]),
         ({"result": fm.FR_APP_ACCEPT, "events": fm.TEV_HEARD, "resp_index": M - 1,
           "append_from": M - 1, "appended": 1}, M - 1, M - 1, (M - 5, 5))),
        ("a truncate one below the top", log_ending_at(M - 1),
         fm.Msg(APP, 1, 6, M - 3, 5, 0, [(1, 6)]),
         ({"result": fm.FR_APP_ACCEPT, "events": fm.TEV_RESET, "resp_index": M - 2,
           "append_from": M - 2, "appended": 1}, M - 2, M - 4, (M - 2, 6))),
        ("a beat committing the last entry", log_ending_at(M - 1),
         fm.Msg(HB, 1, 5, 0, 0, M - 1), None),
        ("a beat committing M", log_ending_at(M - 1), fm.Msg(HB, 1, 5, 0, 0, M), None),
        ("a probe at M", log_ending_at(M - 1), fm.Msg(APP, 1, 5, M, 0, 0), None),
        # four runs of 2^32 - 1 entries: 2^34 - 4 in all, so index + n is M exactly; the
        # model refuses before it expands an entry
        ("index + n == M over four full runs", log_ending_at(M - 1),
         fm.Msg(APP, 1, 5, M - (1 << 34) + 4, 0, 0, [(0xFFFFFFFF, 5)] * 4), None),
    ]
    return rows


FOLLOWER_TOP_RESULTS = [fm.FR_BAD_MSG, fm.FR_APP_ACCEPT, fm.FR_APP_ACCEPT, fm.FR_HEARTBEAT_RESP,
                        fm.FR_COMMIT_PAST_LOG, fm.FR_BAD_MSG, fm.FR_BAD_MSG]


def check_follower_top_row(row, before, after, out):
    """The model's (or, through the harness, the device's) answer to a row
    against the row's literals."""
    _, node, _, want = row
    if want is None:
        return
    wout, last, committed, last_run = want
    assert out == wout, (row[0], out)
    assert (after.last_index(), after.committed, after.runs[-1]) == (last, committed, last_run), row[0]
    if wout["result"] >= fm.FR_REFUSED:
        assert after is before, row[0]  # nothing written


def snap_top_rows(S=3):
    """-> [(id, SNode, SMsg or None, compaction request or None, want)]; want =
    (result, last_index, run_first[0], first_index) or None."""
    M = M64
    conf = lambda: sm.Conf(S, 7, ids=[1, 2, 3])  # noqa: E731
    snap = lambda i: sm.SMsg(sm.SMSG_SNAP, 1, 5, i, 6, inc=7, ids=[1, 2, 3])  # noqa: E731
    done = log_ending_at(M - 1, committed=M - 1)
    return [
        ("a snapshot at M", sm.SNode(log_ending_at(M - 9), conf(), 0, 0), snap(M), None,
         (sm.SR_BAD_MSG, M - 9, M - 12, M - 11)),
        ("a snapshot at M - 1", sm.SNode(log_ending_at(M - 9), conf(), 0, 0), snap(M - 1), None,
         (sm.SR_RESTORED, M - 1, M - 1, M)),
        ("compact at the last index M - 1", sm.SNode(done, conf(), 0, 0), None,
         (M - 1, 0, M - 1), (sm.CP_COMPACTED, M - 1, M - 1, M)),
        ("compact at M", sm.SNode(done, conf(), 0, 0), None, (M, 0, M - 1),
         (sm.CP_OUT_OF_BOUND, M - 1, M - 4, M - 3)),
    ]


def check_snap_top_row(row, after, out):
    want = row[4]
    assert out["result"] == want[0], (row[0], out)
    assert (after.node.last_index(), after.node.runs[0][0], after.first_index) == want[1:], row[0]


def follower_neighbours(rng, groups, R, S, E):
    """Random lifted nodes, each with a message: the surroundings of a hand-built row."""
    ls = lifts(groups)
    small = [fm.gen_node(rng, R, S) for _ in ls]
    return ([follower_node(n, L) for n, L in zip(small, ls)],
            [follower_msg(fm.gen_msg(rng, n, E, S), L) for n, L in zip(small, ls)])


def snap_neighbours(rng, groups, R, S):
    """-> (lifted SNodes, a lifted MsgSnap each, a lifted compaction request each)."""
    ls = lifts(groups)
    small = [sm.gen_snode(rng, R, S) for _ in ls]
    return ([snap_node(n, L) for n, L in zip(small, ls)],
            [snap_msg(sm.gen_smsg(rng, n, S), L) for n, L in zip(small, ls)],
            [compaction(sm.gen_compaction(rng, n), L) for n, L in zip(small, ls)])


# ---- the coverage conditions, per base class ----
def by_class(ls, log, key):
    """{B: set of key(out)}, {T: ...} over every call of a run."""
    seen_b = {b: set() for b in IB}
    seen_t = {t: set() for t in TB}
    for outs in log:
        for L, o in zip(ls, outs):
            seen_b[L.B].add(key(o))
            seen_t[L.T].add(key(o))
    return seen_b, seen_t


def missing(seen, need):
    return {hex(c): sorted(need - s) for c, s in seen.items() if need - s}


def check_follower_coverage(case, ls, log):
    """The result set tests/test_gpu_follower.py's test_random_differential
    requires over the run, and for every B and every T on its own: an accept
    that appends, one that does not, REJECT, STALE, HEARTBEAT_RESP,
    COMMIT_PAST_LOG, and with entries RUNS_FULL and APP_GAP.  (Without
    entries no message appends, fills the table or leaves a gap.)"""
    R, E, flags = case
    seen = {o["result"] for outs in log for o in outs}
    want = {fm.FR_NONE, fm.FR_IGNORED, fm.FR_HEARTBEAT_RESP, fm.FR_APP_ACCEPT, fm.FR_APP_REJECT,
            fm.FR_APP_STALE, fm.FR_BAD_MSG, fm.FR_COMMIT_PAST_LOG}
    want |= {fm.FR_LOWER_TERM_RESP} if flags else set()
    want |= {fm.FR_RUNS_FULL, fm.FR_APP_GAP} if E else set()
    assert want <= seen, sorted(fm.FR_NAMES[c] for c in want - seen)
    need = {(fm.FR_APP_ACCEPT, False), (fm.FR_APP_REJECT, False), (fm.FR_APP_STALE, False),
            (fm.FR_HEARTBEAT_RESP, False), (fm.FR_COMMIT_PAST_LOG, False)}
    if E:
        need |= {(fm.FR_APP_ACCEPT, True), (fm.FR_RUNS_FULL, False), (fm.FR_APP_GAP, False)}
    seen_b, seen_t = by_class(ls, log, lambda o: (o["result"], bool(o.get("append_from"))))
    assert not missing(seen_b, need) and not missing(seen_t, need), \
        (missing(seen_b, need), missing(seen_t, need))


def vote_want(case):
    """The result codes tests/test_vote_model.py proves for the small run."""
    S, R, masks, flags, cand, have_self = case
    if cand and have_self:
        want = set(vm.ALL_RESULTS)
        if not flags & vm.VOTE_CHECK_QUORUM:
            want.discard(vm.VR_IN_LEASE)
        if not flags & vm.VOTE_PREVOTE:
            want.discard(vm.VR_CAMPAIGN_PREVOTE)
    else:
        want = {vm.VR_NONE, vm.VR_IGNORED, vm.VR_GRANT, vm.VR_REJECT, vm.VR_BAD_MSG}
        want |= {vm.VR_IN_LEASE} if flags & vm.VOTE_CHECK_QUORUM else set()
    return want


def check_vote_coverage(case, ls, log):
    _, seen_t = by_class(ls, log, lambda o: o["result"])
    assert not missing(seen_t, vote_want(case)), missing(seen_t, vote_want(case))


def check_snap_coverage(ls, slog, clog):
    seen_b, _ = by_class(ls, slog, lambda o: o["result"])
    need = {sm.SR_RESTORED, sm.SR_FAST_FORWARD, sm.SR_STALE, sm.SR_NOT_MEMBER,
            sm.SR_COMMIT_PAST_LOG}
    assert not missing(seen_b, need), missing(seen_b, need)
    seen_b, _ = by_class(ls, clog, lambda o: o["result"])
    # CREATED / COMPACTED / ALREADY come alone or or-ed together: bit by bit
    bits_b = {b: {bit for r in s if r < sm.CP_REFUSED for bit in (1, 2, 8) if r & bit} |
              {r for r in s if r >= sm.CP_REFUSED} for b, s in seen_b.items()}
    need = {sm.CP_CREATED, sm.CP_COMPACTED, sm.CP_ALREADY, sm.CP_OUT_OF_BOUND, sm.CP_PAST_APPLIED}
    assert not missing(bits_b, need), missing(bits_b, need)
