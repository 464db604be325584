"""qe_ready_note / qe_ready / qe_advance on the device against
tests/ready_model.py.

1. Random differential, all three calls: G = 130 (two tiles and a ragged third;
   the count pass takes a lane per group) and G = 4097 (one full chunk, which
   takes the 16-B pair loads, and the chunk edge of the scan), stride G + 3,
   group_offset 2^33, R in {1, 4, 16}, E in {0, 1, 4}; capacity 0, less than
   the count and exact, the rows past min(count, capacity) byte-identical to
   their fill pattern; random prev rows with None encoded as different values
   >= S; `pending` given and NULL; max_apply 0 and 3; the pad columns and every
   resident row outside the rules' writes compared byte for byte.
2. qe_advance on lists with bad groups, stale terms and out-of-range applies.
3. The all-roles trace replay of tests/test_ready_model.py on the device (the
   engine beside the models, TraceDeviceBackend's comparisons still running):
   base 0 and 61, the 16-bit ring form where RUNS <= 4.
4. A closed loop on tests/cluster_sim: ready + advance every round, a Storage
   per node rebuilt from the records alone (tests/ready_sim.ReadySim).
5. Wide values: the differential of 1 on logs at 2^32 - k, 2^53, 2^63 - k and
   2^64 - 4096 with terms as wide (test_wide_differential), and ranges of 2^32
   entries and more, which a list caps at 0xFFFFFFFF (test_top_of_range)."""
import numpy as np
import pytest
import torch

from tests import cluster_sim as cs
from tests import lift
from tests import ready_model as rdm
from tests import ready_sim as rsim
from tests import trace_cluster as tc
from tests.test_gpu_cluster import DeviceBackend
from tests.test_gpu_outbox import DeviceRandom, same_list, walk_groups
from tests.test_gpu_progress import DEV, eng  # noqa: F401
from tests.test_gpu_trace_cluster import TraceDeviceBackend
from tests.trace_replay import traces

pytestmark = pytest.mark.gpu
GOFF = 1 << 33
FILL = 0xA5
S = 5
RUNS = ("ent_len", "ent_term", "apply_len", "apply_term")
NP = {torch.int64: np.uint64, torch.int32: np.uint32, torch.uint8: np.uint8}


def host(t):
    return t.cpu().numpy().view(NP[t.dtype])


def up(a):
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype, a.dtype)
    return torch.from_numpy(a.view(signed).copy()).to(DEV)


def none_or_slot(rng, n):
    """Slots, and None encoded as different values >= S."""
    v = rng.integers(0, S, n)
    return np.where(rng.random(n) < 0.4, rng.integers(S, 256, n), v).astype(np.uint8)


def random_state(rng, G, R, bases=None, tbases=(0,)):
    """-> (st, rs): valid logs (run_first ascending, run_first[0] <= committed
    <= last_index, run_first[0] <= stable), about half of the groups quiet.
    The dummy index is below 50, or for three groups in ten 2^32 - 3; with
    `bases` it is one of them per group plus a draw below 50, and every
    run_term, term and prev_term lies above one of `tbases` (cycling so that
    every base meets every term base).  Every draw is relative to the group's
    base, so without `bases` the stream is the one it has always been."""
    st_ = G + 3
    u64 = np.uint64
    rf = np.full(R * st_, 0x0E0E0E0E0E0E0E0E, u64)
    rt = np.full(R * st_, 0x0E0E0E0E0E0E0E0E, u64)
    nr = rng.integers(1, R + 1, G).astype(np.uint8)
    last, com = np.zeros(G, u64), np.zeros(G, u64)
    if bases is None:
        base = np.where(rng.random(G) < 0.3, (1 << 32) - 3, rng.integers(0, 50, G)).astype(u64)
    else:
        base = np.array([bases[g % len(bases)] + int(rng.integers(0, 50)) for g in range(G)], u64)
    nb = len(bases) if bases is not None else 1
    for g in range(G):
        f, t = int(base[g]), int(rng.integers(0, 4)) + tbases[(g // nb) % len(tbases)]
        for r in range(int(nr[g])):
            rf[r * st_ + g], rt[r * st_ + g] = f, t
            f += int(rng.integers(1, 5))
            t += int(rng.integers(1, 3))
        last[g] = f - 1 + int(rng.integers(0, 8))
        com[g] = int(base[g]) + int(rng.integers(0, int(last[g]) + 1 - int(base[g])))
    top = np.array([rt[(int(nr[g]) - 1) * st_ + g] for g in range(G)], u64)
    st = rdm.state(num_groups=G, group_offset=GOFF, num_slots=S, stride=st_, log_runs=R,
                   committed=com, last_index=last, run_first=rf, run_term=rt, run_count=nr,
                   term=top + rng.integers(0, 2, G).astype(u64),
                   state=rng.choice([0, 1, 2, 2, 3], G).astype(np.uint8), lead=none_or_slot(rng, G),
                   vote=none_or_slot(rng, G))
    rs = rsim.fresh_rows(G)
    rdm.reset(st, rs)
    rs.applied[:] = com
    # None stays None under another encoding
    for cur, prev in ((st.vote, rs.prev_vote), (st.lead, rs.prev_lead)):
        nn = cur >= S
        prev[nn] = rng.integers(S, 256, int(nn.sum()))
    loud = rng.random(G) < 0.5
    for g in np.flatnonzero(loud):
        b, li, c = int(base[g]), int(last[g]), int(com[g])
        k = rng.integers(0, 8)
        lo = 0 if bases is None else b - min(b, 5)       # (a few indexes below the dummy)
        if k == 0:
            rs.stable[g] = b + int(rng.integers(0, li + 1 - b))
        elif k == 1:
            rs.applied[g] = lo + int(rng.integers(0, c + 2 - lo))  # below the dummy, inside, past committed
        elif k == 2:
            rs.snap_pending[g] = rng.integers(1, 1 << 40)
        elif k == 3:
            rs.prev_term[g] = max(0, int(st.term[g]) - 1)
        elif k == 4:
            rs.prev_commit[g] = lo + int(rng.integers(0, c + 1 - lo))
        elif k == 5:
            rs.prev_vote[g] = rng.integers(0, 256)
        elif k == 6:
            rs.prev_lead[g], rs.prev_state[g] = rng.integers(0, 256), rng.integers(0, 4)
        else:
            rs.stable[g], rs.applied[g] = b, b           # the whole log, to persist and to apply
    return st, rs


class Dev:
    """The state on the device, and every resident tensor for the byte check."""

    def __init__(self, e, st, rs):
        G, R = st.num_groups, st.log_runs
        self.e, self.ps = e, e.ProgressState(G, S, 4, R, DEV, group_offset=GOFF, stride=st.stride)
        self.ps.load_host(committed=st.committed, last_index=st.last_index, run_first=st.run_first,
                          run_term=st.run_term, run_count=st.run_count)
        self.fol = e.Follower(self.ps).load_host(term=st.term, state=st.state, lead=st.lead)
        if st.vote is not None:
            self.fol.load_host(vote=st.vote)
        self.rs = e.ReadyState(self.ps).load_host(**vars(rs))
        ps, f = self.ps, self.fol
        self.resident = {k: getattr(ps, k) for k in ("committed", "last_index", "run_first",
                                                     "run_term", "run_count", "match", "next")}
        self.resident.update({k: getattr(f, k) for k in f.ARRAYS})
        self.resident.update({"rs_" + k: getattr(self.rs, k) for k in self.rs.ARRAYS})

    def snapshot(self):
        return {k: t.clone() for k, t in self.resident.items()}

    def unchanged(self, before, but=()):
        for k, t in self.resident.items():
            if k not in but:
                assert torch.equal(t, before[k]), k

    def same_rows(self, rs):
        for k in rdm.STATE_ROWS:
            np.testing.assert_array_equal(host(getattr(self.rs, k)), getattr(rs, k), err_msg=k)


def filled_ready(e, ps, capacity, E):
    rd = e.Ready(ps, capacity, E)
    for k in rd.ARRAYS:
        t = getattr(rd, k)
        if t is not None and k != "count":
            t.view(torch.uint8).fill_(FILL)
    rd.result.fill_(FILL)
    return rd


def records_of(rd):
    """-> (count, the records the arrays hold, as the model's dicts)."""
    count, rows = rd.records()
    E = rd.ent_runs
    recs = []
    for i in range(min(count, rd.capacity)):
        r = {k: int(rows[k][i]) for k in rdm.FIELDS}
        for name, ln, tm_ in (("ents", "ent_len", "ent_term"), ("apply", "apply_len", "apply_term")):
            runs = [(int(rows[ln][j, i]), int(rows[tm_][j, i])) for j in range(E)]
            used = [x for x in runs if x[0]]
            assert runs == used + [(0, 0)] * (E - len(used)), "unused run rows are 0"
            r[name] = used
        recs.append(r)
    return count, recs


def past_is_fill(rd, n):
    """Nothing at or past n is touched in any output array."""
    cap = max(1, rd.capacity)
    for k in rd.ARRAYS:
        t = getattr(rd, k)
        if t is None or k == "count":
            continue
        a = t.cpu().numpy()
        a = a.reshape(rd.ent_runs, cap)[:, n:] if k in RUNS else a[n:]
        assert (np.ascontiguousarray(a).view(np.uint8) == FILL).all(), k


@pytest.mark.parametrize("E", (0, 1, 4))
@pytest.mark.parametrize("R", (1, 4, 16))
@pytest.mark.parametrize("G", (130, 4097))
def test_random_differential(eng, G, R, E):  # noqa: F811
    rng = np.random.default_rng(1000 * G + 10 * R + E)
    st, rs = random_state(rng, G, R)
    d = Dev(eng, st, rs)
    ps = d.ps
    pend = (rng.random(G) < 0.05).astype(np.uint8) * rng.integers(1, 256, G).astype(np.uint8)
    # ---- qe_ready ----
    full = None
    for pending, max_apply in ((None, 0), (pend, 0), (None, 3), (pend, 3)):
        want, wstats = rdm.ready(st, rs, pending=pending, max_apply=max_apply, ent_runs=E)
        n = len(want)
        assert 0 < n < G
        for cap in (0, n // 2, n):
            rd = filled_ready(eng, ps, cap, E)
            stats = eng.stats_buffer(DEV)
            before = d.snapshot()
            eng.ready(ps, d.fol, d.rs, rd, pending=None if pending is None else up(pending),
                      max_apply=max_apply, stats=stats)
            count, got = records_of(rd)
            assert count == n
            assert got == want[:cap]
            past_is_fill(rd, min(n, cap))
            d.unchanged(before)
            folded = host(eng.stats_reduce(stats))
            for k, v in wstats.items():  # over every listed group, those past capacity too
                assert int(folded[k]) == v, (k, cap)
            if pending is None and max_apply == 0 and cap == n:
                full = rd
    # the flags a cut sets were seen where they can be
    want, _ = rdm.ready(st, rs, max_apply=3, ent_runs=E)
    assert any(r["flags"] & rdm.APPLY_CUT for r in want)
    if E == 1 and R > 1:
        assert any(r["flags"] & rdm.ENTS_CUT for r in want)
    # ---- qe_advance on the list qe_ready left on the device ----
    want, _ = rdm.ready(st, rs, ent_runs=E)
    al = (rng.random(G) < 0.8).astype(np.uint8)
    pci = np.array([rng.integers(0, int(c) + 2) for c in st.committed], np.uint64)
    pci = np.where(rng.random(G) < 0.7, rs.applied, pci)  # (applied-before <= pci)
    before = d.snapshot()
    res = eng.advance(ps, d.rs, full, fol=d.fol, auto_leave=up(al), pending_conf_index=up(pci))
    wres = rdm.advance(st, rs, want, auto_leave=al, pending_conf_index=pci)
    np.testing.assert_array_equal(host(res)[:len(want)], wres)
    assert (host(res)[len(want):] == FILL).all()
    assert rdm.ADV_APPLIED_RANGE in wres and rdm.ADV_OK in wres
    assert any(x & rdm.ADV_AUTO_LEAVE for x in wres)
    d.same_rows(rs)
    d.unchanged(before, but={"rs_" + k for k in rdm.STATE_ROWS})
    # ---- qe_ready_note ----
    fr = rng.choice([0, 1, 3, 4, 4, 4, 5, 6, 17], G).astype(np.uint8)
    af = np.array([rng.integers(0, int(x) + 3) for x in st.last_index], np.uint64)
    sr = rng.choice([0, 0, 2, 4, 5, 5, 17], G).astype(np.uint8)
    ri = rng.integers(1, 1 << 40, G).astype(np.uint64)
    fo, so = eng.FollowerOut(ps), eng.SnapOut(ps)
    fo.load_host(result=fr, append_from=af)
    so.load_host(result=sr, resp_index=ri)
    for kw, mk in ((dict(follow=fo), dict(follow_result=fr, append_from=af)),
                   (dict(snap=so), dict(snap_result=sr, snap_resp_index=ri)),
                   (dict(follow=fo, snap=so), dict(follow_result=fr, append_from=af,
                                                   snap_result=sr, snap_resp_index=ri))):
        before = d.snapshot()
        eng.ready_note(ps, d.rs, **kw)
        rdm.note(st, rs, **mk)
        d.same_rows(rs)
        d.unchanged(before, but={"rs_stable", "rs_snap_pending"})
    # and the Ready after it
    want, _ = rdm.ready(st, rs, ent_runs=E)
    rd = filled_ready(eng, ps, G, E)
    eng.ready(ps, d.fol, d.rs, rd)
    assert records_of(rd) == (len(want), want)


@pytest.mark.parametrize("E", (0, 4))
def test_wide_differential(eng, E):  # noqa: F811
    """qe_ready and qe_advance as in test_random_differential, on logs whose
    dummy index lies at 0, 2^32 - k, 2^53 + 1, 2^63 - k or 2^64 - 4096 and
    whose terms lie above 0, 2^32 - k, 2^63 - k or 2^64 - 4096 (tests/lift.py's
    bases, every index base with every term base): run_cut, rd_flags' applied + 1
    / run_first[0] + 1 / committed + 1 and qe_advance's range checks on words
    whose high dword is live, that cross 2^32 inside a log and pass the int64
    sign bit."""
    G, R = 130, 4
    rng = np.random.default_rng(77000 + E)
    st, rs = random_state(rng, G, R, bases=lift.IB, tbases=lift.TB)
    assert (st.last_index >> np.uint64(63)).any() and (st.term >> np.uint64(63)).any()
    assert ((st.run_first.reshape(R, -1)[0, :G] >> np.uint64(32)) !=
            (st.last_index >> np.uint64(32))).any()  # a log across a dword boundary
    d = Dev(eng, st, rs)
    ps = d.ps
    pend = (rng.random(G) < 0.05).astype(np.uint8) * rng.integers(1, 256, G).astype(np.uint8)
    full = None
    for pending, max_apply in ((None, 0), (pend, 0), (None, 3), (pend, 3)):
        want, wstats = rdm.ready(st, rs, pending=pending, max_apply=max_apply, ent_runs=E)
        n = len(want)
        assert 0 < n < G
        for cap in (n // 2, n):
            rd = filled_ready(eng, ps, cap, E)
            stats = eng.stats_buffer(DEV)
            before = d.snapshot()
            eng.ready(ps, d.fol, d.rs, rd, pending=None if pending is None else up(pending),
                      max_apply=max_apply, stats=stats)
            count, got = records_of(rd)
            assert count == n
            assert got == want[:cap]
            past_is_fill(rd, min(n, cap))
            d.unchanged(before)
            folded = host(eng.stats_reduce(stats))
            for k, v in wstats.items():
                assert int(folded[k]) == v & rdm.M64, (k, cap)
            if pending is None and max_apply == 0 and cap == n:
                full = rd
    want, _ = rdm.ready(st, rs, max_apply=3, ent_runs=E)
    assert any(r["flags"] & rdm.APPLY_CUT for r in want)
    assert any(r["ent_count"] and r["ent_first"] >> 32 for r in want)
    assert any(r["apply_count"] and r["apply_first"] >> 63 for r in want)
    # ---- qe_advance on the list qe_ready left on the device ----
    want, _ = rdm.ready(st, rs, ent_runs=E)
    al = (rng.random(G) < 0.8).astype(np.uint8)
    pci = np.array([int(c) - min(int(c), 2) + int(rng.integers(0, 4)) for c in st.committed],
                   np.uint64)
    pci = np.where(rng.random(G) < 0.7, rs.applied, pci)
    before = d.snapshot()
    res = eng.advance(ps, d.rs, full, fol=d.fol, auto_leave=up(al), pending_conf_index=up(pci))
    wres = rdm.advance(st, rs, want, auto_leave=al, pending_conf_index=pci)
    np.testing.assert_array_equal(host(res)[:len(want)], wres)
    assert (host(res)[len(want):] == FILL).all()
    assert rdm.ADV_APPLIED_RANGE in wres and rdm.ADV_OK in wres
    assert any(x & rdm.ADV_AUTO_LEAVE for x in wres)
    d.same_rows(rs)
    d.unchanged(before, but={"rs_" + k for k in rdm.STATE_ROWS})
    want, _ = rdm.ready(st, rs, ent_runs=E)
    rd = filled_ready(eng, ps, G, E)
    eng.ready(ps, d.fol, d.rs, rd)
    assert records_of(rd) == (len(want), want)


TOP = 0xFFFFFFFF


def top_rows():
    """The hand-built rows of test_top_of_range -> [(id, D, kind, runs)]: a
    range of D entries to persist (kind "ents": stable = the dummy index) or to
    apply ("apply": applied = the dummy index, max_apply 0), over a table of one
    run or of two with the second starting inside the range."""
    rows = []
    for D in (TOP, TOP + 1, TOP + 6, 1 << 33):
        for kind in ("ents", "apply"):
            for two in (True, False):
                rows.append((f"{kind} {D:#x} {'two runs' if two else 'one run'}", D, kind, two))
    return rows


def put_top_row(st, rs, g, row, f0=(1 << 40) + 7):
    _, D, kind, two = row
    s = st.stride
    st.run_first[g], st.run_term[g] = f0, (1 << 32) + 3
    st.run_first[s + g], st.run_term[s + g] = f0 + D // 2 + 3, (1 << 32) + 4
    st.run_count[g] = 2 if two else 1
    st.last_index[g] = f0 + D
    st.term[g] = (1 << 32) + 4
    st.committed[g] = rs.stable[g] = f0 + D if kind == "apply" else f0
    rs.applied[g] = f0
    rs.prev_term[g], rs.prev_commit[g] = st.term[g], st.committed[g]
    rs.snap_pending[g] = 0


def test_top_of_range(eng):  # noqa: F811
    """A list holds 0xFFFFFFFF entries at most (qe_outbox rule 4): ranges of
    2^32 - 1, 2^32, 2^32 + 5 and 2^33 entries to persist and to apply, over one
    table run and over two, each at lane 0, 63, 64 and the last lane of a
    partial tile among random neighbours, with E = 4 and with E = 0, where the
    range stays whole.  The model takes the same cap (tests/test_lift_model.py
    pins it); the literals below hold for the range of 2^32 over one run."""
    G, R = 64 * 2 + 37, 4
    spots = (0, 63, 64, G - 1)
    rng = np.random.default_rng(97)
    for row in top_rows():
        name, D, kind, two = row
        st, rs = random_state(rng, G, R)
        for g in spots:
            put_top_row(st, rs, g, row)
        d = Dev(eng, st, rs)
        for E in (4, 0):
            want, wstats = rdm.ready(st, rs, ent_runs=E)
            rd = filled_ready(eng, d.ps, G, E)
            stats = eng.stats_buffer(DEV)
            eng.ready(d.ps, d.fol, d.rs, rd, stats=stats)
            assert records_of(rd) == (len(want), want), (name, E)
            folded = host(eng.stats_reduce(stats))
            for k, v in wstats.items():
                assert int(folded[k]) == v & rdm.M64, (name, E, k)
            recs = {r["group"] - GOFF: r for r in want}
            for g in spots:
                r = recs[g]
                cnt, runs, cut_bit = ((r["ent_count"], r["ents"], rdm.ENTS_CUT) if kind == "ents"
                                      else (r["apply_count"], r["apply"], rdm.APPLY_CUT))
                assert cnt == (min(D, TOP) if E else D), (name, E)
                assert bool(r["flags"] & cut_bit) == bool(E and D > TOP), (name, E)
                assert sum(n for n, _ in runs) == (cnt if E else 0)
                if E and D == TOP + 1 and not two:
                    assert runs == [(0xFFFFFFFF, (1 << 32) + 3)] and cnt == 0xFFFFFFFF
                    assert r["flags"] & cut_bit


def test_rows_that_rule_out_the_pair_loads(eng):  # noqa: F811
    """A full chunk whose `stable` row is 8-B but not 16-B aligned, and whose
    prev_lead row starts at an odd address: the count pass takes a lane per
    group; a NULL vote row is None everywhere."""
    G, R, E = 4097, 4, 4
    rng = np.random.default_rng(7)
    st, rs = random_state(rng, G, R)
    st.vote = None
    d = Dev(eng, st, rs)
    d.fol.vote = None
    for k, dt in (("stable", torch.int64), ("prev_lead", torch.uint8)):
        t = torch.zeros(G + 1, dtype=dt, device=DEV)
        t[1:].copy_(getattr(d.rs, k))
        setattr(d.rs, k, t[1:])
        assert t[1:].data_ptr() % (16 if dt == torch.int64 else 2)
    want, _ = rdm.ready(st, rs, ent_runs=E)
    rd = filled_ready(eng, d.ps, G, E)
    eng.ready(d.ps, d.fol, d.rs, rd)
    assert records_of(rd) == (len(want), want)
    assert all(r["vote"] == rdm.NONE for r in want)


def test_advance_on_hand_made_lists(eng):  # noqa: F811
    """Lists the host filled: groups below and past the batch, records whose
    last entry has another term by now or lies past the log or at / below
    `stable`, applies past committed and below applied, a snapshot that is no
    longer the pending one.  The results and every row against the model."""
    G, R = 130, 4
    rng = np.random.default_rng(99)
    st, rs = random_state(rng, G, R)
    d = Dev(eng, st, rs)
    recs = []
    for g in rng.permutation(G)[:100]:
        g = int(g)
        li, c, stb = int(st.last_index[g]), int(st.committed[g]), int(rs.stable[g])
        r = dict(group=GOFF + g, term=int(st.term[g]) + 1, commit=c, vote=int(rng.integers(0, S)),
                 lead=int(rng.integers(0, S)), state=int(rng.integers(0, 4)),
                 flags=int(rng.integers(0, 16)), ent_first=stb + 1, ent_count=0, ent_last_term=0,
                 apply_first=0, apply_count=0, snap_index=0)
        k = int(rng.integers(0, 8))
        if k == 0:
            r["group"] = (GOFF - 1, GOFF + G, 5, (1 << 64) - 1)[int(rng.integers(0, 4))]
        elif k == 1 and li > stb:  # the right term, the whole unstable part
            r["ent_count"] = li - stb
            r["ent_last_term"] = rdm.term_at(rdm.runs_of(st, g), li, li)
        elif k == 2 and li > stb:  # a stale term
            r["ent_count"], r["ent_last_term"] = li - stb, 1 << 50
        elif k == 3:               # past the log
            r["ent_count"], r["ent_last_term"] = li - stb + 2, int(st.term[g])
        elif k == 4:               # at or below stable
            r["ent_first"], r["ent_count"] = max(1, stb - 1), 1
            r["ent_last_term"] = rdm.term_at(rdm.runs_of(st, g), li, max(1, stb - 1))
        elif k == 5:               # past committed, or below applied
            r["apply_first"], r["apply_count"] = int(rs.applied[g]) + 1, int(rng.integers(1, 9))
        elif k == 6:
            r["apply_first"], r["apply_count"] = max(1, int(rs.applied[g]) - 3), 1
        else:
            r["flags"] |= rdm.SNAP
            r["snap_index"] = int(rs.snap_pending[g]) or int(rng.integers(0, c + 2))
        recs.append(r)
    lst = eng.Ready(d.ps, len(recs) + 7, 0)
    lst.load_host(**{k: np.array([r[k] for r in recs], np.uint8 if lst.KIND[k] == "u8"
                                 else np.uint64) for k in rdm.FIELDS})
    lst.count.fill_(len(recs))
    lst.result.fill_(FILL)
    before = d.snapshot()
    res = host(eng.advance(d.ps, d.rs, lst))
    want = rdm.advance(st, rs, recs)
    np.testing.assert_array_equal(res[:len(recs)], want)
    assert (res[len(recs):] == FILL).all()
    for x in (rdm.ADV_OK, rdm.ADV_OK_STALE_ENTRIES, rdm.ADV_BAD_GROUP, rdm.ADV_APPLIED_RANGE):
        assert x in want
    d.same_rows(rs)
    d.unchanged(before, but={"rs_" + k for k in rdm.STATE_ROWS})
    # a count past the capacity is clamped
    lst.count.fill_(1 << 40)
    eng.advance(d.ps, d.rs, lst)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# The engine beside the models in the two drivers
# ---------------------------------------------------------------------------
class DeviceReady(rsim.ReadyRows):
    """A mixin over a DeviceBackend: the rows of qe_ready_state on the device
    (`rsd`) beside the model's (`rs`); the note right after the device's
    follower / snapshot call, on its own result rows; qe_ready and qe_advance
    with the model's records and rows as the expectation."""

    rsd = None

    def init_ready(self):
        e = self.e
        self.rs = rsim.start_rows(self)
        self.rsd = e.ReadyState(self.ps).load_host(**vars(self.rs))
        self.rd = e.Ready(self.ps, self.p.G, cs.MSG_RUNS)
        self.ready_calls = self.ready_records = 0

    def timed(self, f, *a, **kw):
        r = super().timed(f, *a, **kw)
        if self.rsd is not None:
            if f is self.e.follower_step:
                self.e.ready_note(self.ps, self.rsd, follow=a[3])
            elif f is self.e.snapshot_step:
                self.e.ready_note(self.ps, self.rsd, snap=a[4])
        return r

    def same_rows(self):
        for k in rdm.STATE_ROWS:
            np.testing.assert_array_equal(host(getattr(self.rsd, k)), getattr(self.rs, k),
                                          err_msg=k)

    def follow(self, msgs):
        outs = super().follow(msgs)
        self.same_rows()
        return outs

    def snap(self, msgs):
        outs = super().snap(msgs)
        self.same_rows()
        return outs

    def list_ready(self, pending=None):
        want = super().list_ready(pending)
        self.e.ready(self.ps, self.fol, self.rsd, self.rd,
                     pending=None if pending is None else up(pending))
        count, got = records_of(self.rd)
        assert (count, got) == (len(want), want)
        self.ready_calls += 1
        self.ready_records += count
        self.listed_all = got
        return got

    def advance_ready(self, recs):
        want = super().advance_ready(recs)
        if recs is self.listed_all:  # the device's own list, consumed where it lies
            lst = self.rd
        else:                        # a list the host filled
            lst = self.e.Ready(self.ps, max(1, len(recs)), 0)
            lst.load_host(**{k: np.array([r[k] for r in recs],
                                         np.uint8 if lst.KIND[k] == "u8" else np.uint64)
                             for k in rdm.FIELDS})
            lst.count.fill_(len(recs))
        got = host(self.e.advance(self.ps, self.rsd, lst))[:len(recs)]
        np.testing.assert_array_equal(got, want)
        self.same_rows()
        return list(got)


class ReadyTraceDevice(DeviceReady, TraceDeviceBackend):
    WORLD = rsim.ReadyTraceWorld

    def __init__(self, engine, p):
        super().__init__(engine, p)
        self.init_ready()


RING32 = [(name, base, False) for name in tc.MANDATORY for base in (0, 61)]
RING16 = [(name, 61, True) for name in tc.MANDATORY if tc.RUNS[name] <= 4]


@pytest.mark.parametrize("name,base,ring16", RING32 + RING16)
def test_ready_blocks_on_device(eng, name, base, ring16):  # noqa: F811
    tr = traces()[name]
    p = tc.params(name, tr, G=130, gbase=base, goff=GOFF, ring16=ring16)
    be = ReadyTraceDevice(eng, p)
    r = rsim.ReadyReplay(name, tr, be, rsim.ready_blocks()).run()
    assert r.compared == rsim.BLOCKS[name] == r.checked["readies"] == be.ready_calls
    print(f"{name} base {base} ring16 {ring16}: {r.compared} Ready blocks from "
          f"{be.ready_records} records, compared {dict(r.checked)}")


class ReadyClusterDevice(DeviceReady, DeviceBackend):
    def __init__(self, engine, p):
        super().__init__(engine, p)
        self.init_ready()


class DeviceReadySim(rsim.ReadySim):
    def resident(self):
        be, p = self.be, self.p
        term, vote, com, last, nr = (host(t) for t in (be.fol.term, be.fol.vote, be.ps.committed,
                                                       be.ps.last_index, be.ps.run_count))
        rf, rt = (host(t).reshape(p.R, p.stride) for t in (be.ps.run_first, be.ps.run_term))
        hard, logs = [], []
        for g in range(p.G):
            v = int(vote[g])
            hard.append((int(term[g]), v if v < p.N else rdm.NONE, int(com[g])))
            runs = [(int(rf[r, g]), int(rt[r, g])) for r in range(int(nr[g]))]
            li = int(last[g])
            logs.append([(i, rdm.term_at(runs, li, i)) for i in range(runs[0][0], li + 1)])
        return hard, logs


# row "a" of tests/cluster_sim.py, reduced: 6 clusters of 3, the 16-bit ring
# form, every index crossing 2^32, 36 rounds of a faulty network and 30 to heal
LOOP = cs.ROWS["a"].but(C=6, fault_rounds=36, heal_rounds=30, p_compact=0.05)


def test_closed_loop_storage_from_the_records(eng):  # noqa: F811
    p = LOOP
    s = DeviceReadySim(p, ReadyClusterDevice(eng, p)).run()
    ref = rsim.ReadySim(p, rsim.ClusterReadyModel(p)).run()
    assert s.seen == ref.seen and s.counters()["cov"] == ref.counters()["cov"]
    print(f"closed loop: G {p.G}, {p.fault_rounds + p.heal_rounds} rounds, {dict(s.seen)}, "
          f"{s.be.ready_calls} qe_ready calls")
    assert s.seen["truncations"] and s.seen["snapshots"] and s.seen["applied"] and s.seen["hard"]


def test_fill_blocks_walk(eng):  # noqa: F811
    """test_fill_blocks_walk of tests/test_gpu_outbox.py for qe_ready: a quiet
    batch of one chunk more than the capped fill grid has blocks, with a
    sparse set of groups that have entries to persist, entries to apply or a
    new HardState."""
    e, L = eng, eng._lib
    G, R, E = walk_groups(), 1, 1
    rnd = DeviceRandom(G, 0x0EAD)
    ps = e.ProgressState(G, 1, 1, R, DEV, group_offset=GOFF)
    ps.run_first[:G], ps.run_term[:G], ps.run_count[:] = 5, 3, 1
    ps.last_index.copy_(7 + rnd.ints(0, 12))
    ps.committed.fill_(6)
    fol = e.Follower(ps)
    fol.term.copy_(3 + rnd.ints(0, 3))
    rs = e.ReadyState(ps).reset(ps, fol)
    rs.applied.copy_(ps.committed)
    ents, apply, hard = rnd.hit(0.005), rnd.hit(0.005), rnd.hit(0.005)
    rs.stable.sub_(ents.to(torch.int64))        # Entries: the last one
    rs.applied.sub_(apply.to(torch.int64))      # CommittedEntries: index 6
    rs.prev_term.sub_(hard.to(torch.int64))     # a new term: HardState, MustSync
    cap = int((ents | apply | hard).sum().item()) + 5
    lists = []
    for stats in (None, e.stats_buffer(DEV)):
        rd = e.Ready(ps, cap, E)
        e.ready(ps, fol, rs, rd, stats=stats)
        lists.append(rd)
    n = same_list(lists[0], lists[1], RUNS, E)
    assert n == cap - 5
    folded = e.stats_reduce(stats)
    a = lists[0]
    want = {0: n,  # QE_STAT_GROUPS: the record count
            L.QE_STAT_READY_MUST_SYNC: int(((a.flags[:n] & L.QE_RD_MUST_SYNC) != 0).sum().item()),
            L.QE_STAT_READY_ENTRIES: int(a.ent_count[:n].sum().item()),
            L.QE_STAT_READY_APPLY: int(a.apply_count[:n].sum().item())}
    for stat, v in want.items():
        assert int(folded[stat].item()) == v > 0, ("stat", stat)
