"""qe_tick on the GPU, bit for bit against tests/tick_model.py: every state
array, every output and the folded statistics after each of a run of
consecutive ticks, over random states, masks, events and host reactions; the
rows a tick has no business with stay untouched; CheckQuorum and the beat
agree with the existing oracle's; ticks = 0, sharding, compaction."""
import numpy as np
import pytest
import torch

from oracle import orc
from tests import tick_model as tm
from tests.test_gpu_progress import (DEV, EXTRAS, RING_MASK, eng, random_queue,  # noqa: F401
                                     random_state, to_device)

pytestmark = pytest.mark.gpu
READS = EXTRAS + ("reads",)
ET, HT = 4, 2
SENT = 0x0E0E0E0E0E0E0E0E  # prefill of the outputs: what a tick leaves alone keeps it
SHAPES = [(1, ()), (3, ()), (5, ()), (5, ("inc",)), (9, ("inc", "out")), (16, ("inc", "out"))]


def make_case(rng, G, S, masks, cq, goff=0, seed=77):
    """A random leader-side state with a ReadIndex queue, and the model of
    its tick state: all four raft states, timers anywhere below their
    timeouts, 10 % of the groups not promotable (self_slot untracked, a
    learner, or >= S), 10 % with a pending snapshot; group 0 a follower that
    can never campaign, its electionElapsed one short of saturation."""
    pb = random_state(rng, G, S, 4, 1, masks, EXTRAS)
    random_queue(rng, pb)
    md = orc.mask_dtype(S)
    self_slot = rng.integers(0, S, G)
    bit = (1 << self_slot).astype(np.int64)
    trk = pb.tracked.astype(np.int64) | bit
    inc = None if pb.inc is None else pb.inc.astype(np.int64) | bit
    kind = np.where(rng.random(G) < 0.1, rng.integers(1, 4, G), 0)
    kind[0] = 3
    trk = np.where(kind == 1, trk & ~bit, trk)
    if inc is not None:
        inc = np.where(kind == 2, inc & ~bit, inc)
        pb.inc = inc.astype(md)
        if pb.out is not None:
            pb.out = np.where(kind == 2, pb.out & ~bit.astype(md), pb.out).astype(md)
    pb.tracked = trk.astype(md)
    pb.self_slot = np.where(kind == 3, np.where(rng.random(G) < 0.5, 0xFF, S), self_slot).astype(np.uint8)
    m = tm.Model(G, S, ET, HT, cq, seed=seed, goff=goff, stride=pb.stride)
    m.state[:] = rng.integers(0, 4, G)
    m.ee[:] = rng.integers(0, ET, G)
    m.he[:] = rng.integers(0, HT, G)
    m.rt[:] = rng.integers(ET, 2 * ET, G)
    m.no_campaign[:] = rng.random(G) < 0.1
    m.state[0], m.ee[0] = tm.FOLLOWER, 65534
    link(m, pb)
    return pb, m


def link(m, pb):
    """The model's view of the leader state in pb (copies)."""
    i64 = lambda a: None if a is None else a.astype(np.int64)  # noqa: E731
    m.peer, m.match, m.committed = pb.pw.copy(), pb.match.copy(), pb.committed.copy()
    m.inc, m.out, m.tracked = i64(pb.inc), i64(pb.out), i64(pb.tracked)
    m.self_slot = None if pb.self_slot is None else pb.self_slot.copy()
    m.lead_transferee = None if pb.lead_transferee is None else pb.lead_transferee.copy()
    m.read_head = None if pb.read_head is None else pb.read_head.copy()
    m.read_count = None if pb.read_count is None else pb.read_count.copy()


def to_gpu(engine, pb, m, masks, extras=READS):
    ps = to_device(engine, pb, masks, extras)
    ps.group_offset = m.goff
    t = engine.Timers(m.G, m.et, m.ht, m.check_quorum, m.seed, DEV)
    t.load_host(state=m.state, election_elapsed=m.ee, heartbeat_elapsed=m.he,
                randomized_timeout=m.rt.astype(np.uint16), no_campaign=m.no_campaign)
    return ps, t


def gpu_tick(engine, ps, t, events=None, ticks=1, beats=True):
    out = engine.TickOut(ps, beats=beats)
    if beats:
        out.hb_commit.fill_(SENT)
        out.hb_ctx.fill_(SENT & 0xFFFFFFFF)
    out.quorum_active.fill_(SENT & 0xFF)
    st = engine.stats_buffer(DEV)
    ev = None if events is None else torch.from_numpy(events).to(DEV)
    engine.tick(ps, t, out, st, events=ev, ticks=ticks)
    return out, engine.stats_reduce(st).cpu().numpy().view(np.uint64)


def same(got, want, what):
    np.testing.assert_array_equal(got, want, err_msg=what)


def assert_tick(ps, t, out, stats, m, mo, peer_before):
    """Device state and outputs equal to the model's; -> the device's peer
    words (raw, with their ring representation bits)."""
    h = t.host()
    same(h["state"], m.state, "state")
    same(h["timer"], m.timer(), "timer")
    same(h["randomized_timeout"], m.rt.astype(np.uint16), "randomized_timeout")
    md = orc.mask_dtype(m.S)
    if m.lead_transferee is not None:
        same(ps.lead_transferee.cpu().numpy(), m.lead_transferee, "lead_transferee")
    peer = ps.peer.cpu().numpy().view(np.uint32)
    same(peer & ~RING_MASK, m.peer, "peer words")
    # groups whose check did not run: not a bit of their words moved
    quiet = np.tile((mo.action & tm.CHECKED_QUORUM) == 0, m.S)
    cols = np.arange(m.S * m.stride) % m.stride < m.G
    same(peer[cols][quiet], peer_before[cols][quiet], "peer words of unchecked groups")
    same(out.action.cpu().numpy(), mo.action, "action")
    same(out.quorum_active.cpu().numpy(), mo.quorum_active, "quorum_active")
    same(out.hb_sent.cpu().numpy().view(md), mo.hb_sent, "hb_sent")
    if out.hb_commit is not None:
        same(out.hb_ctx.cpu().numpy().view(np.uint32), mo.hb_ctx, "hb_ctx")
        same(out.hb_commit.cpu().numpy().view(np.uint64), mo.hb_commit, "hb_commit")
    same(stats, mo.stats, "stats")
    return peer


def react(rng, m, mo, ps, t):
    """What a host does between ticks, on the model and (with the same masks,
    in place, so the next tick still sees this tick's stores) on the device:
    half the groups told to campaign win and lead, the others stand as
    candidates -- either way reset() is reported back; some peers are heard
    from (RecentActive); some leaders start a transfer."""
    G, S = m.G, m.S
    hup = (mo.action & tm.HUP) != 0
    win = hup & (rng.random(G) < 0.5)
    new_state = np.where(win, tm.LEADER, np.where(hup, tm.CANDIDATE, m.state)).astype(np.uint8)
    heard = (rng.random((S, G)) < 0.3)
    lt_on = (m.state == tm.LEADER) & (rng.random(G) < 0.1)
    lt = np.where(lt_on, rng.integers(0, S, G), m.lead_transferee).astype(np.uint8)
    m.state[:] = new_state
    m.peer.reshape(S, m.stride)[:, :G][heard] |= np.uint32(tm.RECENT_ACTIVE)
    m.lead_transferee[:] = lt
    if ps is not None:
        dev = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
        t.state.copy_(dev(new_state))
        ps.peer.view(S, ps.stride)[:, :G][dev(heard)] |= tm.RECENT_ACTIVE
        ps.lead_transferee.copy_(dev(lt))
    return hup  # reported as QE_TEV_RESET with the next tick


def run_ticks(engine, rng, pb, m, masks, nticks=2 * ET + 3):
    """nticks consecutive ticks with random events; engine None runs the model
    alone (the coverage conditions are the model's).  -> the coverage seen."""
    ps, t = to_gpu(engine, pb, m, masks) if engine else (None, None)
    peer = ps.peer.cpu().numpy().view(np.uint32) if engine else None
    seen = set()
    acts = set()
    reset = np.zeros(m.G, bool)
    for k in range(nticks):
        r = rng.random(m.G)
        events = np.where(r < 0.8, 0, np.where(r < 0.9, 1, np.where(r < 0.97, 2, 3))).astype(np.uint8)
        events[reset] |= tm.TEV_RESET
        events[0] = 0
        if engine:
            out, stats = gpu_tick(engine, ps, t, events)
        mo = m.tick(events, out=tm.TickOut(m, SENT))
        if engine:
            peer = assert_tick(ps, t, out, stats, m, mo, peer)
            assert t.tick_no == m.tick_no == k + 1
        acts |= set(int(x) for x in np.unique(mo.action))
        if m.refused_by_snapshot.any():
            seen.add("hup refused by no_campaign alone")
        reset = react(rng, m, mo, ps, t)
        if engine:  # (the words as the host's reaction left them)
            peer = ps.peer.cpu().numpy().view(np.uint32)
    for bit, name in ((tm.HUP, "hup"), (tm.BEAT, "beat"), (tm.CHECKED_QUORUM, "checked"),
                      (tm.STEPDOWN, "stepdown"), (tm.TRANSFER_ABORTED, "aborted")):
        if any(a & bit for a in acts):
            seen.add(name)
    if any(a & tm.CHECKED_QUORUM and a & tm.BEAT for a in acts):
        seen.add("checked and beat")
    if any(a & tm.STEPDOWN and not a & tm.BEAT for a in acts):
        seen.add("stepdown without beat")
    assert not any(a & tm.STEPDOWN and a & tm.BEAT for a in acts)
    if any(a & tm.TRANSFER_ABORTED and a & tm.STEPDOWN for a in acts):
        seen.add("aborted by the stepdown")
    if any(a & tm.TRANSFER_ABORTED and not a & tm.STEPDOWN for a in acts):
        seen.add("aborted by the timeout")
    if m.ee[0] >= 0xFFFF and m.timer()[0] & 0xFFFF == 0xFFFF:
        seen.add("saturated")
    return seen


def wanted(S, cq):
    w = {"hup", "beat", "saturated", "hup refused by no_campaign alone"}
    if S > 1:  # (a single slot is the leader's own: nobody to transfer to)
        w |= {"aborted", "aborted by the timeout"}
    if cq:
        w |= {"checked", "checked and beat"}
        if S > 1:  # (a singleton's quorum is always active)
            w |= {"stepdown", "stepdown without beat", "aborted by the stepdown"}
    return w


def case_rng(S, masks, cq, G):
    return np.random.default_rng(5000 + 100 * S + 10 * len(masks) + int(cq) + G)


@pytest.mark.parametrize("cq", [True, False])
@pytest.mark.parametrize("S,masks", SHAPES)
def test_tick_random_differential(eng, S, masks, cq):  # noqa: F811
    G = 4099
    rng = case_rng(S, masks, cq, G)
    pb, m = make_case(rng, G, S, masks, cq)
    seen = run_ticks(eng, rng, pb, m, masks)
    assert wanted(S, cq) <= seen, wanted(S, cq) - seen


@pytest.mark.parametrize("G", [1, 63, 64, 65])
def test_tick_small_batches(eng, G):  # noqa: F811
    S, masks = 5, ("inc",)
    rng = case_rng(S, masks, True, G)
    pb, m = make_case(rng, G, S, masks, True)
    run_ticks(eng, rng, pb, m, masks)


@pytest.mark.parametrize("S,masks,extras", [(3, (), ()), (5, ("inc",), EXTRAS),
                                            (9, ("inc", "out"), EXTRAS)])
def test_tick_agrees_with_check_quorum_and_heartbeat(eng, S, masks, extras):  # noqa: F811
    """Every group a leader one tick short of both timeouts: the tick's
    CheckQuorum is orc.check_quorum's and its beat orc.heartbeat's (on the
    groups that stay leaders), the existing oracle being a second witness."""
    rng = np.random.default_rng(640 + S)
    G = 4099
    pb = random_state(rng, G, S, 4, 1, masks, extras)
    random_queue(rng, pb)
    ps = to_device(eng, pb, masks, tuple(extras) + ("reads",))
    t = eng.Timers(G, ET, HT, True, 5, DEV)
    t.load_host(state=np.full(G, tm.LEADER, np.uint8), election_elapsed=ET - 1,
                heartbeat_elapsed=HT - 1)
    out = eng.TickOut(ps)
    eng.tick(ps, t, out)
    qa, _ = orc.check_quorum(pb)  # (rewrites pb.pw)
    commit, ctx, sent = orc.heartbeat(pb)
    act = out.action.cpu().numpy()
    lt0 = pb.lead_transferee if pb.lead_transferee is not None else np.full(G, 0xFF, np.uint8)
    want = np.where(qa == 1, tm.CHECKED_QUORUM | tm.BEAT, tm.CHECKED_QUORUM | tm.STEPDOWN) | \
        np.where(lt0 < S, tm.TRANSFER_ABORTED, 0)
    same(act, want, "action")
    same(out.quorum_active.cpu().numpy(), qa, "quorum_active")
    same(ps.peer.cpu().numpy().view(np.uint32) & ~RING_MASK, pb.pw, "peer words")
    on = qa == 1
    assert 0 < on.sum() < G
    md = orc.mask_dtype(S)
    same(out.hb_sent.cpu().numpy().view(md), np.where(on, sent, 0), "hb_sent")
    same(out.hb_ctx.cpu().numpy().view(np.uint32)[on], ctx[on], "hb_ctx")
    got = out.hb_commit.cpu().numpy().view(np.uint64).reshape(S, ps.stride)[:, :G]
    same(got, np.where(on[None, :], commit.reshape(S, pb.stride)[:, :G], 0), "hb_commit")
    same(t.state.cpu().numpy(), np.where(on, tm.LEADER, tm.FOLLOWER), "state")


def test_tick_events_only(eng):  # noqa: F811
    """ticks = 0: the events are applied, nothing ticks, action is all 0."""
    rng = np.random.default_rng(71)
    G, S, masks = 1000, 3, ()
    pb, m = make_case(rng, G, S, masks, True)
    ps, t = to_gpu(eng, pb, m, masks)
    peer = ps.peer.cpu().numpy().view(np.uint32)
    events = rng.integers(0, 4, G).astype(np.uint8)
    out, stats = gpu_tick(eng, ps, t, events, ticks=0)
    ee, he, rt = m.ee.copy(), m.he.copy(), m.rt.copy()
    mo = m.tick(events, out=tm.TickOut(m, SENT), ticks=0)
    assert_tick(ps, t, out, stats, m, mo, peer)
    assert not mo.action.any() and t.tick_no == 0
    assert (m.ee[events == 0] == ee[events == 0]).all() and (m.ee[events != 0] == 0).all()
    assert (m.he[events < 2] == he[events < 2]).all() and (m.rt[events < 2] == rt[events < 2]).all()


def shard(pb, a, b):
    """Groups [a, b) of a ProgressBatch as a batch of their own."""
    G, S, F, R = pb.G, pb.S, pb.F, pb.R
    sb = orc.ProgressBatch(b - a, S, F, R)
    for k, rows in (("match", S), ("next", S), ("pending", S), ("pw", S), ("ibuf", S * F),
                    ("run_first", R), ("run_term", R)):
        setattr(sb, k, np.ascontiguousarray(getattr(pb, k).reshape(rows, pb.stride)[:, a:b]).reshape(-1))
    for k in ("committed", "term_start", "first_index", "last_index", "run_count", "inc", "out",
              "tracked", "self_slot", "lead_transferee", "snap_index", "read_acks", "read_head",
              "read_count"):
        v = getattr(pb, k)
        setattr(sb, k, None if v is None else v[a:b].copy())
    sb.read_cap = pb.read_cap
    return sb


def test_tick_sharded(eng):  # noqa: F811
    """The same 4099 groups as two calls (group_offset 0 and 2048): the same
    arrays and the same summed statistics -- the draw and the checksum depend
    on the global group id alone.  Every group draws (QE_TEV_RESET)."""
    S, masks, G, cut = 5, ("inc",), 4099, 2048
    rng = np.random.default_rng(4242)
    pb, m = make_case(rng, G, S, masks, True)
    events = np.full(G, tm.TEV_RESET, np.uint8)
    ps, t = to_gpu(eng, pb, m, masks)
    out, stats = gpu_tick(eng, ps, t, events)
    whole = {k: v.copy() for k, v in t.host().items()}
    parts, total = [], np.zeros(16, np.uint64)
    for a, b in ((0, cut), (cut, G)):
        sb = shard(pb, a, b)
        sm = tm.Model(b - a, S, ET, HT, True, seed=m.seed, goff=a, stride=sb.stride)
        # (m has not ticked: its tick state is still the initial one)
        sm.state[:], sm.ee[:], sm.he[:], sm.rt[:] = m.state[a:b], m.ee[a:b], m.he[a:b], m.rt[a:b]
        sm.no_campaign[:] = m.no_campaign[a:b]
        link(sm, sb)
        sps, st = to_gpu(eng, sb, sm, masks)
        assert sps.group_offset == a
        so, sst = gpu_tick(eng, sps, st, events[a:b])
        parts.append((st.host(), so, sps))
        total += sst
    same(total, stats, "summed stats")
    for k in ("state", "timer", "randomized_timeout"):
        same(np.concatenate([p[0][k] for p in parts]), whole[k], k)
    same(np.concatenate([p[1].action.cpu().numpy() for p in parts]), out.action.cpu().numpy(), "action")
    same(np.concatenate([p[1].hb_sent.cpu().numpy() for p in parts]), out.hb_sent.cpu().numpy(), "hb_sent")
    same(np.concatenate([p[2].lead_transferee.cpu().numpy() for p in parts]),
         ps.lead_transferee.cpu().numpy(), "lead_transferee")
    pw = np.concatenate([p[2].peer.cpu().numpy().reshape(S, -1) for p in parts], axis=1)
    same(pw, ps.peer.cpu().numpy().reshape(S, -1), "peer words")
    # and the whole is the model's
    mo = m.tick(events, out=tm.TickOut(m, SENT))
    same(stats, mo.stats, "stats")
    same(whole["randomized_timeout"], m.rt.astype(np.uint16), "randomized_timeout")


def test_tick_actions_compact(eng):  # noqa: F811
    """engine.collect on `action` lists exactly the groups with something to
    do: the tick composes with the Ready-delta path."""
    S, masks, G = 3, (), 4099
    rng = np.random.default_rng(99)
    pb, m = make_case(rng, G, S, masks, True)
    ps, t = to_gpu(eng, pb, m, masks)
    out = eng.tick(ps, t, eng.TickOut(ps, beats=False))
    act = out.action.cpu().numpy()
    groups, vals = eng.collect(out.action, values=t.timer.to(torch.int64))
    same(groups.cpu().numpy(), np.nonzero(act)[0], "collected groups")
    same(vals.cpu().numpy(), t.timer.cpu().numpy().astype(np.int64)[act != 0], "collected timers")
    mo = m.tick(None, out=tm.TickOut(m))
    same(act, mo.action, "action")
    assert 0 < len(groups) < G


def test_tick_walking_waves(eng):  # noqa: F811
    """One tick in which every wave walks two or three tiles (tests/walk.py):
    statistics on, a group offset past 2^32, a stride that is no multiple of
    64.  The state generator steps a group at a time, so the state is 209
    groups repeated; the model is vectorised and runs at the full size, with
    events of its own for every group."""
    from tests import walk
    S, masks = walk.S, ()
    G = walk.walk_groups(torch.cuda.get_device_properties(DEV).multi_processor_count)
    stride, idx = G + walk.PAD, np.arange(G) % walk.PERIOD
    rng = np.random.default_rng(2095)
    pb, m0 = make_case(rng, walk.PERIOD, S, masks, True)

    def rows(a):
        big = np.zeros((S, stride), a.dtype)
        big[:, :G] = a.reshape(S, walk.PERIOD)[:, idx]
        return big.reshape(-1)
    m = tm.Model(G, S, ET, HT, True, seed=77, goff=walk.GOFF, stride=stride)
    for k in ("state", "ee", "he", "rt", "no_campaign"):
        getattr(m, k)[:] = getattr(m0, k)[idx]
    m.peer, m.match, m.committed = rows(pb.pw), rows(pb.match), pb.committed[idx]
    m.tracked = pb.tracked.astype(np.int64)[idx]
    m.self_slot, m.lead_transferee = pb.self_slot[idx], pb.lead_transferee[idx]
    m.read_head, m.read_count = pb.read_head[idx], pb.read_count[idx]
    ps = eng.ProgressState(G, S, 1, 4, DEV, stride=stride, group_offset=walk.GOFF, extras=READS)
    ps.peer.copy_(torch.from_numpy(m.peer.view(np.int32)))  # (the rings are not the tick's)
    ps.load_host(match=m.match, committed=m.committed, tracked=m.tracked.astype(np.uint8),
                 self_slot=m.self_slot, lead_transferee=m.lead_transferee,
                 read_head=m.read_head, read_count=m.read_count)
    t = eng.Timers(G, ET, HT, True, m.seed, DEV)
    t.load_host(state=m.state, election_elapsed=m.ee, heartbeat_elapsed=m.he,
                randomized_timeout=m.rt.astype(np.uint16), no_campaign=m.no_campaign)
    r = rng.random(G)
    events = np.where(r < 0.8, 0, np.where(r < 0.9, 1, np.where(r < 0.97, 2, 3))).astype(np.uint8)
    peer = ps.peer.cpu().numpy().view(np.uint32)
    out, stats = gpu_tick(eng, ps, t, events)
    mo = m.tick(events, out=tm.TickOut(m, SENT))
    assert_tick(ps, t, out, stats, m, mo, peer)
    assert stats[tm.ST_GROUPS] == G and stats[tm.ST_ELECTIONS] and stats[tm.ST_STEPDOWNS]
