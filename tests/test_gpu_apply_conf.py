"""qe_apply_conf on the GPU against the sequential model (tests/
apply_conf_model.py, pinned to the reference's traces by
tests/test_apply_conf_model.py):

(a) the 21 applied conf changes of the interaction traces on the device, the
    trace's group at a position in each of the three tiles of a 135-group
    batch, and qe_advance's QE_ADV_AUTO_LEAVE after every leader record;
(b) random lists of 2 * kBlock + 3 records, runs of 1-4 records per group,
    named slots mixed with QE_AC_ANY_SLOT, random roles, both ring forms, the
    configuration rows shared with the Progress state and apart from it;
(c) the same state through qe_apply_conf and through the host-row path
    (qe_confchange + qe_switch_config): byte-identical state and qe_outbox
    records;
(d) every refusal next to a record that still applies, DEFERRED and its
    resubmission, a capacity below n, two calls back to back on one scratch.
"""
import numpy as np
import pytest
import torch

from tests import apply_conf_model as acm
from oracle import confchange_ref as cc
from oracle import orc
from tests.test_gpu_progress import DEV, EXTRAS, assert_same, random_state, ring16_state, to_device

pytestmark = pytest.mark.gpu
G, GOFF, KBLOCK = 64 * 2 + 7, 1000, 256
MASKS = ("inc", "out")
LEADER, FOLLOWER, CANDIDATE = 2, 0, 1  # QE_STATE_*
OUT_KEYS = ("result", "cc_result", "sw_result", "inc", "out", "learner", "learners_next", "tracked",
            "new_progress", "auto_leave")


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from etcd_amd import engine
    assert engine._lib.QE_STATE_LEADER == LEADER
    return engine


def random_changer(rng, S, pool):
    """A random valid tracker.Config placed in random slots."""
    ch = acm.SlotChanger(S)
    k = int(rng.integers(1, min(S, len(pool)) + 1))
    ids = [int(i) for i in rng.choice(pool, k, replace=False)]
    slots = [int(s) for s in rng.choice(S, k, replace=False)]
    ch.slots = dict(zip(ids, slots))
    nv = int(rng.integers(1, k + 1))
    voters, rest = ids[:nv], ids[nv:]
    learners, out, lnext = set(rest), set(), set()
    if rng.random() < 0.3:  # joint
        only_out, learners = set(rest[: len(rest) // 2]), set(rest[len(rest) // 2:])
        out = only_out | {v for v in voters if rng.random() < 0.5}
        out = out or {voters[0]}
        lnext = {i for i in only_out if rng.random() < 0.5}
        ch.cfg.auto_leave = bool(rng.random() < 0.5)
    ch.cfg.inc, ch.cfg.out, ch.cfg.learners, ch.cfg.lnext = set(voters), out, learners, lnext
    ch.prs = {i: cc.Progress(1, i in learners) for i in ids}
    return ch


class Case:
    """One resident state on the device and in the model."""

    def __init__(self, eng, rng, S, changers, state, self_slot, F=4, ring16=False, share=True,
                 max_changes=3):
        self.eng, self.S, self.C = eng, S, max_changes
        md = orc.mask_dtype(S)
        pb = random_state(rng, G, S, F, 3, MASKS, EXTRAS, max_ents=2)
        if ring16:
            ring16_state(rng, pb)
        pb.inc = np.array([c.mask(c.cfg.inc) for c in changers], md)
        pb.out = np.array([c.mask(c.cfg.out) for c in changers], md)
        pb.tracked = np.array([c.mask(c.prs) for c in changers], md)
        pb.self_slot = np.asarray(self_slot, np.uint8)
        pb.lead_transferee = np.where(rng.random(G) < 0.5, 0xFF, rng.integers(0, S, G)).astype(np.uint8)
        self.pb = pb
        self.ps = ps = to_device(eng, pb, MASKS, EXTRAS)
        ps.group_offset = GOFF
        self.cs = cs = eng.ConfState(G, S, DEV)
        h = self.conf_rows(changers)
        cs.slot_ids.copy_(torch.from_numpy(h["slot_ids"].T.reshape(-1).copy().view(np.int64)))
        for k in cs.MASKS:
            getattr(cs, k).copy_(torch.from_numpy(h[k].view(np.int16 if S > 8 else np.uint8)))
        cs.auto_leave.copy_(torch.from_numpy(h["auto_leave"]))
        self.share = share
        if share:  # one row serves the configuration and the Progress state
            ps.inc, ps.out, ps.tracked = cs.inc, cs.out, cs.tracked
        self.fol = eng.Follower(ps)
        self.state = np.asarray(state, np.uint8)
        self.fol.load_host(state=self.state, term=np.full(G, 3, np.uint64))
        self.model = acm.Model(G, S, goff=GOFF, max_changes=max_changes, pb=pb)
        self.model.changers = changers
        self.model.leader = [bool(s == LEADER) for s in state]

    def conf_rows(self, changers):
        md = orc.mask_dtype(self.S)
        st = [c.conf_state() for c in changers]
        h = {k: np.array([s[m] for s in st], md) for k, m in (
            ("inc", "inc"), ("out", "out"), ("learner", "learner"),
            ("learners_next", "learners_next"), ("tracked", "tracked"))}
        h["is_learner"] = np.array([c.mask(i for i, p in c.prs.items() if p.is_learner)
                                    for c in changers], md)
        h["auto_leave"] = np.array([s["auto_leave"] for s in st], np.uint8)
        h["slot_ids"] = np.array([s["ids"] for s in st], np.uint64).reshape(len(changers), self.S)
        return h

    def new_list(self, records, capacity=None, scratch_of=None):
        cap = len(records) if capacity is None else capacity
        ac = self.eng.ApplyConf(self.ps, cap, max_changes=self.C)
        m = len(records)
        typ, node = np.zeros((self.C, m), np.uint8), np.zeros((self.C, m), np.uint64)
        slot = np.full((self.C, m), 0xFF, np.uint8)
        for j, (_, _, _, ccs) in enumerate(records):
            for k, (t, n, s) in enumerate(ccs):
                typ[k, j], node[k, j], slot[k, j] = t, n, s
        ac.load_host(group=np.array([r[0] for r in records], np.uint64),
                     transition=np.array([r[1] for r in records], np.uint8),
                     num_changes=np.array([r[2] for r in records], np.uint8),
                     type=typ, node_id=node, slot=slot)
        if scratch_of is not None:
            ac.scratch = scratch_of.scratch
        return ac

    def check_records(self, ac, want):
        n, rec = ac.records()
        assert min(n, ac.capacity) == len(want)
        for k in OUT_KEYS:
            np.testing.assert_array_equal(rec[k].astype(np.int64), [r[k] for r in want], err_msg=k)
        np.testing.assert_array_equal(rec["ids"].T, np.array([r["ids"] for r in want], np.uint64)
                                      .reshape(len(want), self.S), err_msg="ids")

    def check_state(self, sw=None, o=None):
        md = orc.mask_dtype(self.S)
        got, want = self.cs.host(), self.conf_rows(self.model.changers)
        for k, w in want.items():
            np.testing.assert_array_equal(got[k], w, err_msg=f"conf {k}")
        for k in ("inc", "out", "tracked"):  # the Progress state's view, shared or not
            np.testing.assert_array_equal(getattr(self.ps, k).cpu().numpy().view(md),
                                          getattr(self.pb, k), err_msg=f"progress {k}")
        assert_same(self.ps, self.pb)
        if sw is not None:
            np.testing.assert_array_equal(sw.result.cpu().numpy(), o.result, err_msg="sw result")
            np.testing.assert_array_equal(sw.sent.cpu().numpy().view(md), o.sent, err_msg="sent")
            np.testing.assert_array_equal(sw.snap.cpu().numpy().view(md), o.snap, err_msg="snap")

    def run(self, records, capacity=None):
        """One call on the device and in the model, everything compared."""
        ac = self.new_list(records, capacity)
        sw = self.eng.Switch(self.ps)
        self.eng.apply_conf(self.ps, self.fol, self.cs, ac, sw)
        want = self.model.apply(records, capacity)
        o = self.model.switch(want)
        self.check_records(ac, want)
        self.check_state(sw, o)
        return want, sw


def idle_case(eng, rng, S, placed, **kw):
    """Every group idle (one voter, a follower) but `placed`: {g: (changer,
    state, self id)}."""
    changers, state, self_slot = [], [], []
    for g in range(G):
        if g in placed:
            ch, st, me = placed[g]
            ch = acm.SlotChanger(S, ch.cfg.clone(), {i: p.copy() for i, p in ch.prs.items()},
                                 ch.slots)
        else:
            ch, st, me = acm.SlotChanger(S), FOLLOWER, 1
            ch.cfg.inc, ch.prs, ch.slots = {1}, {1: cc.Progress(1, False)}, {1: 0}
        changers.append(ch)
        state.append(st)
        self_slot.append(ch.slots.get(me, 0xFF))
    return Case(eng, rng, S, changers, state, self_slot, **kw)


# ---- (a) the trace pin on the device -----------------------------------------

def test_trace_changes_on_device(eng):
    """The 21 applied changes of the traces, each on the node's configuration
    as the CPU pin left it, the group at g = 5, 64 + 7 and 128 + 3.  After a
    leader's record qe_advance, with auto_leave pointing at the row just
    written, reports QE_ADV_AUTO_LEAVE for exactly the three lines after which
    the trace prints "initiating automatic transition"."""
    from tests import test_apply_conf_model as pin
    S = pin.S
    L = eng._lib
    rng = np.random.default_rng(77)
    applied, auto_left, leaders = 0, 0, 0
    for name, kind, nid, text, _, _, leads, before, t, ccs in pin.walk():
        if kind != "applied":
            continue
        placed = {g: (before, LEADER if leads else FOLLOWER, nid) for g in (5, 64 + 7, 128 + 3)}
        case = idle_case(eng, rng, S, placed)
        # a log in which the change is applicable: committed covers index 1
        recs = [(GOFF + g, t, len(ccs), ccs) for g in sorted(placed)]
        want, _ = case.run(recs)
        for r in want:
            assert r["result"] == (acm.LEADER if leads else acm.APPLIED)
        for g in placed:
            assert case.model.changers[g].cfg.string() == text, (name, nid)
        applied += 1
        if not leads:
            continue
        leaders += 1
        ps = case.ps
        ps.committed.clamp_(min=1)
        rs = eng.ReadyState(ps)
        rd = eng.Ready(ps, 3, ent_runs=0)
        rd.load_host(group=np.array([GOFF + g for g in sorted(placed)], np.uint64),
                     apply_first=np.ones(3, np.uint64), apply_count=np.ones(3, np.uint64),
                     count=np.array([3], np.uint64))
        pci = torch.ones(G, dtype=torch.int64, device=DEV)
        res = eng.advance(ps, rs, rd, fol=case.fol, auto_leave=case.cs.auto_leave,
                          pending_conf_index=pci).cpu().numpy()
        flagged = bool(res[0] & L.QE_ADV_AUTO_LEAVE)
        assert all(bool(x & L.QE_ADV_AUTO_LEAVE) == flagged for x in res)
        assert all((x & L.QE_ADV_OUTCOME) == L.QE_ADV_OK for x in res)
        assert flagged == text.endswith(" autoleave"), (name, text)
        auto_left += flagged
    assert applied == 21 and leaders == 11 and auto_left == 3


# ---- (b) random differential ---------------------------------------------------

def random_records(rng, S, C, pools):
    """2 * kBlock + 3 records over all G groups: 5 runs of one record, 4 of two,
    2 of three, the rest of four."""
    lens = np.full(G, 4)
    pick = rng.choice(np.arange(1, G - 1), 11, replace=False)
    lens[pick[:5]], lens[pick[5:9]], lens[pick[9:]] = 1, 2, 3
    assert lens.sum() == 2 * KBLOCK + 3
    recs = []
    for g in range(G):
        for _ in range(lens[g]):
            tr = int(rng.choice([0, 0, 0, 0, 1, 2, 3 if rng.random() < 0.1 else 0]))
            cnt = int(rng.choice([0, 1, 1, 1, 2, 3, C + 1 if rng.random() < 0.1 else 1]))
            ccs = []
            for _ in range(min(cnt, C)):
                r = rng.random()
                t = (cc.ADD_NODE if r < 0.4 else cc.ADD_LEARNER_NODE if r < 0.65 else
                     cc.REMOVE_NODE if r < 0.9 else cc.UPDATE_NODE if r < 0.98 else 7)
                node = 0 if rng.random() < 0.03 else int(rng.choice(pools[g]))
                slot = 0xFF if rng.random() < 0.5 else int(rng.integers(0, S + 1))
                ccs.append((t, node, slot))
            recs.append((GOFF + g, tr, cnt, ccs))
    return recs


@pytest.mark.parametrize("S,ring16,share", [(3, False, False), (3, True, True), (8, False, True),
                                            (8, True, False), (9, False, False), (9, True, True),
                                            (16, False, True)])
def test_random_differential(eng, S, ring16, share):
    """Two calls in a row on one state (the second works on what the first
    left, deferred records and all): every per-record byte and ConfState, every
    conf row, every Progress row, the rings, sent / snap and the switch
    results equal the model's."""
    rng = np.random.default_rng(5000 + 10 * S + ring16)
    pools = [[10_000 * (g + 1) + k for k in range(S + 2)] for g in range(G)]
    changers = [random_changer(rng, S, pools[g]) for g in range(G)]
    state = rng.choice([FOLLOWER, CANDIDATE, LEADER, LEADER], G)
    self_slot = []
    for ch in changers:  # the node itself: mostly a voter, sometimes a learner or no member
        voters = sorted(ch.cfg.inc | ch.cfg.out)
        r = rng.random()
        self_slot.append(ch.slots[int(rng.choice(voters))] if r < 0.85 else
                         int(rng.integers(0, S + 2)))
    case = Case(eng, rng, S, changers, state, self_slot, F=4 if ring16 else 5, ring16=ring16,
                share=share)
    seen, sw_seen = set(), set()
    for _ in range(2):
        want, _ = case.run(random_records(rng, S, case.C, pools))
        seen |= {r["result"] for r in want}
        seen |= {("cc", r["cc_result"]) for r in want}
        sw_seen |= {r["sw_result"] & 0xF for r in want if r["result"] == acm.LEADER}
    assert {acm.APPLIED, acm.LEADER, acm.DEFERRED, acm.BAD_CHANGE, acm.CHANGER_ERROR,
            acm.SKIPPED} <= seen, seen
    assert ("cc", cc.ERR_NO_SLOT) in seen and {3, 4} & sw_seen, (seen, sw_seen)


# ---- (c) equivalence with the host-row path ------------------------------------

def test_equals_confchange_then_switch_config(eng):
    """One record per group, no named slot: qe_apply_conf on one copy of a
    state, rows built on the host + qe_confchange + qe_switch_config on
    another.  Byte-identical rows, results and qe_outbox records."""
    S, C = 5, 3
    rng = np.random.default_rng(31)
    pools = [[100 * (g + 1) + k for k in range(S + 2)] for g in range(G)]
    seed = rng.integers(1 << 30)
    cases = []
    for _ in range(2):
        r2 = np.random.default_rng(seed)
        changers = [random_changer(r2, S, pools[g]) for g in range(G)]
        state = r2.choice([FOLLOWER, LEADER], G)
        self_slot = [ch.slots[sorted(ch.cfg.inc)[0]] for ch in changers]
        cases.append(Case(eng, r2, S, changers, state, self_slot, share=True, max_changes=C))
    a, b = cases
    groups = {int(g) for g in rng.choice(G, 100, replace=False)} | {0, G - 1}
    recs = []
    for g in sorted(groups):
        tr = int(rng.choice([0, 0, 1, 2]))
        cnt = int(rng.integers(0, C + 1))
        ccs = [(int(rng.choice([0, 1, 3])), int(rng.choice(pools[g])), 0xFF) for _ in range(cnt)]
        recs.append((GOFF + g, tr, cnt, ccs))
    next_before = a.ps.next.clone()
    want, sw_a = a.run(recs)
    # the parent's path on b: op / count / type / node_id / last_index rows, then switched
    ch = eng.ConfChanges(G, S, C, DEV)
    op, cnt = np.zeros(G, np.uint8), np.zeros(G, np.uint8)
    typ, node = np.zeros((C, ch.stride), np.uint8), np.zeros((C, ch.stride), np.uint64)
    for gid, tr, n, ccs in recs:
        g = gid - GOFF
        op[g], cnt[g] = acm.decode(tr, n), n
        for k, (t, i, _) in enumerate(ccs):
            typ[k, g], node[k, g] = t, i
    ch.op.copy_(torch.from_numpy(op))
    ch.count.copy_(torch.from_numpy(cnt))
    ch.type.copy_(torch.from_numpy(typ.reshape(-1)))
    ch.node_id.copy_(torch.from_numpy(node.reshape(-1).view(np.int64)))
    ch.last_index.copy_(b.ps.last_index)
    eng.confchange(b.cs, ch, b.ps)
    ok = (ch.result.cpu().numpy() == 0) & (op != 0)
    switched = torch.from_numpy((ok & (b.state == LEADER)).astype(np.uint8)).to(DEV)
    sw_b = eng.switch_config(b.ps, eng.Switch(b.ps, switched))
    ha, hb = a.ps.host(), b.ps.host()
    for k in ha:
        if ha[k] is not None:
            np.testing.assert_array_equal(ha[k], hb[k], err_msg=k)
    ca, cb = a.cs.host(), b.cs.host()
    for k in ca:
        np.testing.assert_array_equal(ca[k], cb[k], err_msg=k)
    for k in ("result", "sent", "snap"):
        assert torch.equal(getattr(sw_a, k), getattr(sw_b, k)), k
    by_group = {r["group"]: r for r in want}
    res_b = ch.result.cpu().numpy()
    for gid, r in by_group.items():
        assert r["cc_result"] == res_b[gid - GOFF]
    outs = []
    for c, sw in ((a, sw_a), (b, sw_b)):
        ob = eng.Outbox(c.ps, 4 * G)
        eng.outbox(c.ps, c.fol.term, ob, sent=sw.sent, snap=sw.snap, next_before=next_before)
        outs.append(ob.records())
    assert outs[0][0] == outs[1][0] and outs[0][0] > 0
    for k, v in outs[0][1].items():
        if v is not None:
            np.testing.assert_array_equal(v, outs[1][1][k], err_msg=f"outbox {k}")


# ---- (d) refusals --------------------------------------------------------------

def three_voters(S=8):
    ch = acm.SlotChanger(S)
    ch.cfg.inc, ch.slots = {1, 2, 3}, {1: 0, 2: 1, 3: 2}
    ch.prs = {i: cc.Progress(1, False) for i in (1, 2, 3)}
    return ch


def add(g, node, slot=0xFF):
    return (GOFF + g, acm.AUTO, 1, [(cc.ADD_NODE, node, slot)])


def test_refusals_deferred_capacity_and_back_to_back(eng):
    S = 8
    rng = np.random.default_rng(9)
    placed = {g: (three_voters(), LEADER if g in (40, 70) else FOLLOWER, 1)
              for g in (0, 10, 20, 30, 40, 50, 60, 70, 134)}
    case = idle_case(eng, rng, S, placed)
    leave = lambda g: (GOFF + g, acm.AUTO, 0, [])  # noqa: E731  (not joint: NOT_JOINT)
    recs = [
        add(0, 4),                                    # APPLIED (the first group)
        add(20, 4), add(20, 5),                       # APPLIED, APPLIED: a follower's run
        add(10, 4), add(10, 5),                       # BAD_ORDER, SKIPPED: group 10 untouched
        add(30, 4), (GOFF + 30, 3, 1, [(0, 5, 0xFF)]), add(30, 6),  # APPLIED, BAD_CHANGE, SKIPPED
        add(40, 4, 3), add(40, 5), add(40, 6),        # LEADER, DEFERRED, DEFERRED
        leave(50), add(50, 4),                        # CHANGER_ERROR (state untouched), SKIPPED
        add(60, 4, 1), add(60, 5),                    # NO_SLOT from a named tracked slot, SKIPPED
        (GOFF + 60 + 1, acm.AUTO, 4, [(0, 7, 0xFF)] * 3),  # BAD_CHANGE: count > max_changes
        add(70, 9, 4),                                # LEADER, in a non-lowest slot
        (GOFF + G, acm.AUTO, 1, [(0, 4, 0xFF)]),      # BAD_GROUP
        (5, acm.AUTO, 1, [(0, 4, 0xFF)]),             # BAD_ORDER (and below group_offset)
        add(134, 4),                                  # APPLIED (the last group)
    ]
    want, _ = case.run(recs)
    res = [r["result"] for r in want]
    assert res == [acm.APPLIED, acm.APPLIED, acm.APPLIED, acm.BAD_ORDER, acm.SKIPPED,
                   acm.APPLIED, acm.BAD_CHANGE, acm.SKIPPED, acm.LEADER, acm.DEFERRED,
                   acm.DEFERRED, acm.CHANGER_ERROR, acm.SKIPPED, acm.CHANGER_ERROR, acm.SKIPPED,
                   acm.BAD_CHANGE, acm.LEADER, acm.BAD_GROUP, acm.BAD_ORDER, acm.APPLIED]
    assert want[11]["cc_result"] == cc.ERR_NOT_JOINT and want[13]["cc_result"] == cc.ERR_NO_SLOT
    m = case.model.changers
    assert m[10].cfg.inc == {1, 2, 3} and m[50].cfg.inc == {1, 2, 3} and m[60].cfg.inc == {1, 2, 3}
    assert m[40].slots[4] == 3 and m[70].slots[9] == 4
    # the resubmission of the deferred records completes, one per call
    want, _ = case.run([add(40, 5), add(40, 6)])
    assert [r["result"] for r in want] == [acm.LEADER, acm.DEFERRED]
    want, _ = case.run([add(40, 6)])
    assert [r["result"] for r in want] == [acm.LEADER] and m[40].cfg.inc == {1, 2, 3, 4, 5, 6}
    # capacity < n: the records past the capacity are not applied
    ac = case.new_list([add(0, 5), add(20, 6), add(134, 5)], capacity=2)
    assert ac.n == 3 and ac.result.numel() == 2
    case.eng.apply_conf(case.ps, case.fol, case.cs, ac)  # (no sw: its rows go to the scratch)
    want = case.model.apply([add(0, 5), add(20, 6), add(134, 5)], capacity=2)
    case.model.switch(want)
    case.check_records(ac, want)
    case.check_state()
    assert 5 not in m[134].cfg.inc
    # two calls back to back on one scratch, no host work between them: the
    # second call's switch runs on its own groups only
    l1, l2 = [add(40, 7), add(50, 4)], [add(60, 4), add(70, 8)]
    ac1 = case.new_list(l1)
    ac2 = case.new_list(l2)
    sw1, sw2 = eng.Switch(case.ps), eng.Switch(case.ps)
    eng.apply_conf(case.ps, case.fol, case.cs, ac1, sw1)
    ac2.scratch = ac1.scratch
    eng.apply_conf(case.ps, case.fol, case.cs, ac2, sw2)
    w1 = case.model.apply(l1)
    o1 = case.model.switch(w1)
    w2 = case.model.apply(l2)
    o2 = case.model.switch(w2)
    case.check_records(ac1, w1)
    case.check_records(ac2, w2)
    np.testing.assert_array_equal(sw1.result.cpu().numpy(), o1.result)
    case.check_state(sw2, o2)
    assert o2.result[40] == 0 and o2.result[70] != 0 and o1.result[40] != 0
