"""tests/lift.py on the models alone.

1. Commutation: for each of the four models, lower(step(lift(x), lift(m))) ==
   step(x, m), the state and every output field, over random small cases and
   every (B, T).  The GPU differentials run the models on the wide inputs
   directly; this pins that the wide cases are the small ones moved, not some
   other set.  A message whose small index is >= 2^64 - 2 is clamped by the
   lift and left out.
2. Coverage: each lifted run the GPU tests make meets its conditions on the
   model alone, so no GPU test passes by seeing nothing."""
import numpy as np
import pytest

from tests import follower_model as fm
from tests import lift
from tests import snapshot_model as sm
from tests import vote_model as vm

PAIRS = [(b, t) for b in lift.IB for t in lift.TB]


def node_key(n):
    return (n.ents, n.runs, n.committed, n.term, n.state, n.lead, n.vote, n.transferee)


def snode_key(sn):
    return node_key(sn.node) + (sn.conf.key(), sn.self_slot, sn.snap_index, sn.first_index)


def test_the_pairs_cycle_through_every_combination():
    n = len(lift.IB) * len(lift.TB)
    assert {lift.pair(g) for g in range(n)} == set(PAIRS) and len(PAIRS) == 30
    assert all(lift.pair(g) == lift.pair(g + n) for g in range(n))
    # per class at least 100 groups of a run, at every tile position class
    assert lift.G // len(lift.IB) >= 100 and lift.G % 64 == 25


def test_lower_inverts_lift():
    rng = np.random.default_rng(1)
    for g in range(300):
        L = lift.Lift(*PAIRS[g % 30])
        n = fm.gen_node(rng, 4, 5)
        assert node_key(lift.follower_node(lift.follower_node(n, L), L.inv())) == node_key(n)
        sn = sm.gen_snode(rng, 4, 5)
        assert snode_key(lift.snap_node(lift.snap_node(sn, L), L.inv())) == snode_key(sn)
        v = vm.gen_node(rng, 4, 5)
        w = lift.vote_node(lift.vote_node(v, L), L.inv())
        assert node_key(w) == node_key(v) and w.key() == v.key()


def test_follower_step_commutes():
    rng = np.random.default_rng(5)
    tot, seen = 0, set()
    for g in range(6000):
        R, E = int(rng.choice([1, 4, 16])), int(rng.choice([0, 1, 4]))
        L = lift.Lift(*PAIRS[g % 30])
        n = fm.gen_node(rng, R, 5)
        m = fm.gen_msg(rng, n, E, 5)
        if m.index >= fm.M64 - 1:
            continue
        n1, o1 = fm.step(n, m, 3, 5, R)
        n2, o2 = fm.step(lift.follower_node(n, L), lift.follower_msg(m, L), 3, 5, R)
        assert lift.follower_out(o2, L.inv()) == o1, (L.B, L.T, vars(m))
        assert node_key(lift.follower_node(n2, L.inv())) == node_key(n1), (L.B, L.T, vars(m))
        tot += 1
        seen.add(o1["result"])
    assert tot > 5900 and seen >= set(fm.FR_NAMES) - {fm.FR_CONFLICT_COMMITTED}


def test_vote_step_commutes():
    rng = np.random.default_rng(6)
    seen = set()
    for g in range(3000):
        S, R, masks, flags, cand, have_self = vm.RUN_CASES[g % len(vm.RUN_CASES)]
        L = lift.Lift(*PAIRS[(g // len(vm.RUN_CASES)) % 30])
        n = vm.gen_node(rng, R, S, masks)
        m = vm.gen_msg(rng, n, S)
        n1, o1 = vm.step(n, m, flags, S, 10, cand, have_self)
        n2, o2 = vm.step(lift.vote_node(n, L), lift.vote_msg(m, L), flags, S, 10, cand, have_self)
        assert lift.vote_out(o2, L.inv()) == o1, (L.B, L.T, m)
        w = lift.vote_node(n2, L.inv())
        assert node_key(w) == node_key(n1) and w.key() == n1.key(), (L.B, L.T, m)
        seen.add(o1["result"])
    assert seen == vm.ALL_RESULTS


def test_snapshot_step_and_compact_commute():
    rng = np.random.default_rng(7)
    seen_s, seen_c = set(), set()
    for g in range(3000):
        S, R = lift.SNAP_CASES[g % 3]
        L = lift.Lift(*PAIRS[(g // 3) % 30])
        sn = sm.gen_snode(rng, R, S)
        m = sm.gen_smsg(rng, sn, S)
        n1, o1 = sm.step(sn, m, S, R)
        n2, o2 = sm.step(lift.snap_node(sn, L), lift.snap_msg(m, L), S, R)
        assert lift.snap_out(o2, L.inv()) == o1, (L.B, L.T, vars(m))
        assert snode_key(lift.snap_node(n2, L.inv())) == snode_key(n1), (L.B, L.T, vars(m))
        seen_s.add(o1["result"])
        req = sm.gen_compaction(rng, n1)
        c1, p1 = sm.compact(n1, *req)
        c2, p2 = sm.compact(lift.snap_node(n1, L), *lift.compaction(req, L))
        assert lift.compact_out(p2, L.inv()) == p1, (L.B, L.T, req)
        assert snode_key(lift.snap_node(c2, L.inv())) == snode_key(c1), (L.B, L.T, req)
        seen_c.add(p1["result"])
    assert seen_s == set(sm.SR_NAMES)
    assert {sm.CP_CREATED, sm.CP_COMPACTED, sm.CP_OUT_OF_BOUND, sm.CP_PAST_APPLIED} <= seen_c


def test_top_of_range_rows_on_the_model():
    """The hand-built rows of the GPU tests' test_top_of_range: the model's
    answers are the rows' literals and, row by row, the result codes of
    lift.FOLLOWER_TOP_RESULTS."""
    got = []
    for row in lift.follower_top_rows():
        after, out = fm.step(row[1], row[2], 0, 3, 8)
        lift.check_follower_top_row(row, row[1], after, out)
        got.append(out["result"])
    assert got == lift.FOLLOWER_TOP_RESULTS
    for row in lift.snap_top_rows():
        _, sn, msg, req, _ = row
        after, out = sm.step(sn, msg, 3, 8) if msg is not None else sm.compact(sn, *req)
        lift.check_snap_top_row(row, after, out)


def test_ready_cut_caps_a_list_at_2_32_minus_1_entries():
    """qe_outbox rule 4's cap in tests/ready_model.cut: the range is (i, min(hi,
    i + 0xFFFFFFFF)], so every listed length fits a uint32."""
    from tests import ready_model as rdm
    top = 0xFFFFFFFF
    for d in (top, top + 1, top + 6, 1 << 33):
        assert rdm.cut([(10, 7)], 10 + d, 10, 10 + d, 4) == [(top, 7)]
        half = d // 2 + 3  # the second run's offset: past the cap for d = 2^33
        want = [(half - 1, 7), (top - (half - 1), 8)] if half - 1 < top else [(top, 7)]
        assert rdm.cut([(10, 7), (10 + half, 8)], 10 + d, 10, 10 + d, 4) == want
    assert rdm.cut([(10, 7)], 10 + top - 1, 10, 10 + top - 1, 4) == [(top - 1, 7)]


# ---------------------------------------------------------------------------
# The lifted runs of the GPU differentials meet their coverage conditions.
# ---------------------------------------------------------------------------
def wide_words(ls, log, keys):
    """Whether some group's outputs put a bit above bit 31 into one of `keys`."""
    return any(o.get(k, 0) >> 32 for outs in log for o in outs for k in keys)


@pytest.mark.parametrize("case", lift.FOLLOWER_CASES, ids=str)
def test_follower_run_coverage(case):
    ls, log = lift.follower_run(case)
    lift.check_follower_coverage(case, ls, log)
    assert wide_words(ls, log, ("resp_index", "reject_hint", "resp_log_term", "append_from"))


@pytest.mark.parametrize("case", vm.RUN_CASES, ids=str)
def test_vote_run_coverage(case):
    ls, log = lift.vote_run(case)
    lift.check_vote_coverage(case, ls, log)
    assert wide_words(ls, log, ("resp_term", "req_log_term"))


@pytest.mark.parametrize("case", lift.SNAP_CASES, ids=str)
def test_snapshot_run_coverage(case):
    ls, slog, clog = lift.snap_run(case)
    lift.check_snap_coverage(ls, slog, clog)
    assert wide_words(ls, slog, ("resp_index",)) and wide_words(ls, clog, ("snap_term",))
