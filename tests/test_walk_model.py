"""The vectorised checksum restatements the walking-wave GPU tests compare
with (tests/walk.py), pinned to the models' scalar group_stats / step_stats /
compact_stats over the 209 base groups, at group ids past 2^32; and the
helpers that repeat a base."""
import numpy as np

from tests import follower_model as fm
from tests import snapshot_model as sm
from tests import vote_model as vm
from tests import walk

GID = [walk.GOFF + 7 * g for g in range(walk.PERIOD)]


def pin(hashes, scalar):
    """scalar[j]: the model's stats dict of base group j at group id GID[j]."""
    assert hashes.dtype == np.uint64 and len(hashes) == walk.PERIOD
    assert [int(h) for h in hashes] == [s[walk.CSUM] for s in scalar]
    assert len(set(int(h) for h in hashes)) == walk.PERIOD


def test_follower_hashes():
    b = walk.follower_base()
    want = fm.pack_nodes(b.after, walk.R, walk.PERIOD)
    res = np.array([o["result"] for o in b.outs], np.uint8)
    pin(walk.follower_hashes(want, res, np.array(GID, np.uint64)),
        [fm.group_stats(g, n, n2, o) for g, n, n2, o in zip(GID, b.nodes, b.after, b.outs)])
    assert {fm.FR_APP_ACCEPT, fm.FR_APP_REJECT, fm.FR_HEARTBEAT_RESP, fm.FR_NONE} <= set(res)
    assert any(s and s[fm.STAT_APPENDED] for s in b.shares)


def test_vote_hashes():
    b = walk.vote_base()
    want = vm.pack_nodes(b.after, walk.R, walk.S, walk.PERIOD)
    res = np.array([o["result"] for o in b.outs], np.uint8)
    ev = np.array([o["events"] for o in b.outs], np.uint8)
    pin(walk.vote_hashes(want, res, ev, np.array(GID, np.uint64)),
        [vm.group_stats(g, n2, o) for g, n2, o in zip(GID, b.after, b.outs)])
    assert {vm.VR_GRANT, vm.VR_REJECT, vm.VR_PENDING, vm.VR_WON, vm.VR_NONE} <= set(res)


def test_snapshot_hashes():
    b = walk.snap_base()
    want = sm.pack_snodes(b.after, walk.R, walk.S, walk.PERIOD)
    res = np.array([o["result"] for o in b.outs], np.uint8)
    pin(walk.snap_hashes(want, res, np.array(GID, np.uint64)),
        [sm.step_stats(g, n, n2, o) for g, n, n2, o in zip(GID, b.nodes, b.after, b.outs)])
    assert {sm.SR_RESTORED, sm.SR_FAST_FORWARD, sm.SR_STALE, sm.SR_NONE} <= set(res)


def test_compact_hashes():
    b = walk.compact_base()
    want = sm.pack_snodes(b.after, walk.R, walk.S, walk.PERIOD)
    res = np.array([o["result"] for o in b.outs], np.uint8)
    pin(walk.compact_hashes(want, res, np.array(GID, np.uint64)),
        [sm.compact_stats(g, n2, o) for g, n2, o in zip(GID, b.after, b.outs)])
    assert {sm.CP_COMPACTED, sm.CP_CREATED, sm.CP_NONE} <= set(res)
    assert any(o.get("rstar") for o in b.outs)  # a table that moves down


def test_repeat_and_expected_stats():
    """repeat() has period PERIOD and keeps the pad columns; expect_stats over
    one period and a ragged second one is the scalar sum."""
    b = walk.follower_base()
    G, stride = walk.PERIOD + 30, walk.PERIOD + 30 + walk.PAD
    want = walk.repeat(fm.pack_nodes(b.after, walk.R, walk.PERIOD), G, stride,
                       {"run_first": walk.R, "run_term": walk.R}, fill=walk.SENT)
    assert np.array_equal(want["term"][walk.PERIOD:], want["term"][:30])
    rf = want["run_first"].reshape(walk.R, stride)
    assert np.array_equal(rf[:, walk.PERIOD:G], rf[:, :30]) and (rf[:, G:] == walk.SENT).all()
    res = np.array([o["result"] for o in b.outs], np.uint8)[np.arange(G) % walk.PERIOD]
    got = walk.expect_stats(b.shares, G, walk.follower_hashes(want, res))
    ws = {}
    for g in range(G):
        j = g % walk.PERIOD
        if b.shares[j] is not None:
            for k, v in fm.group_stats(walk.GOFF + g, b.nodes[j], b.after[j], b.outs[j]).items():
                ws[k] = (ws.get(k, 0) + v) & fm.M64
    assert [int(x) for x in got] == [ws.get(k, 0) for k in range(16)]
    assert walk.walk_groups(256) == (2 * 8192 + 2) * 64 + 21
