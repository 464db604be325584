"""qe_outbox on the device against tests/outbox_model.py on random states:
every record array up to min(count, capacity), count and the statistics; the
outputs are prefilled with the sentinel of tests/test_gpu_cluster.py and
everything past the written prefix must keep it; the resident state must be
byte-identical before and after.

The shapes: G = 1 (one lane), 63 (a ragged single tile), 65 (a ragged second
tile) and 3 chunks + 65 (three scan chunks, the chunk being the 4096 groups the
library is built with); S = 1, 3, 5 (8-bit masks) and 16 (16-bit); log_runs 1,
4, 16 (the three run-table buckets) and msg_runs 0, 1, 4; stride = G + 3;
group_offset 2^33; indices straddling 2^32."""
import zlib

import numpy as np
import pytest
import torch

from tests import outbox_model as om

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 0x0E0E0E0E0E0E0E0E
CHUNK = 4096  # kListChunk (etcd_amd/csrc/qe_list.hpp), checked in test_chunk_size
BIG = 3 * CHUNK + 65
GOFF = 1 << 33
NP = {torch.int64: np.uint64, torch.int32: np.uint32, torch.int16: np.uint16, torch.uint8: np.uint8}


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from etcd_amd import engine
    return engine


def put(t, a):
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32,
              np.dtype(np.uint16): np.int16}.get(a.dtype, a.dtype)
    t.copy_(torch.from_numpy(a.view(signed).reshape(-1).copy()).to(t.device))
    return t


def dev(a):
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32,
              np.dtype(np.uint16): np.int16}.get(a.dtype, a.dtype)
    return torch.from_numpy(a.view(signed).reshape(-1).copy()).to(DEV)


def host(t):
    return t.cpu().numpy().view(NP[t.dtype])


def random_case(rng, G, S, R, density, kinds, src, bad=0.04):
    """-> (the resident rows, the inputs) as numpy arrays."""
    st = G + 3
    base = (1 << 32) - 40
    nr = rng.integers(1, R + 1, G)
    r0 = base + rng.integers(0, 20, G)
    rf = np.full((R, st), SENT, np.uint64)
    rt = np.full((R, st), SENT, np.uint64)
    first, term = r0.copy(), rng.integers(1, 4, G)
    for r in range(R):
        rf[r, :G], rt[r, :G] = first, term
        first = first + rng.integers(1, 12, G)
        term = term + rng.integers(1, 4, G)
    live = np.arange(R)[:, None] < nr[None, :]
    rf[:, :G][~live], rt[:, :G][~live] = SENT, SENT  # rows past run_count are not state
    last = rf[nr - 1, np.arange(G)].astype(np.int64) + rng.integers(0, 12, G)
    committed = r0 + (rng.random(G) * (last - r0 + 1)).astype(np.int64)
    snap_index = np.where(rng.random(G) < 0.1, r0 - 2, r0 + rng.integers(0, 3, G))

    def index_rows(shift):
        """[S][st] indices inside [r0, last] (+ shift), a few percent outside."""
        x = r0[None, :] + (rng.random((S, G)) * (last - r0 + 1)[None, :]).astype(np.int64)
        x = np.where(rng.random((S, G)) < 0.15, last[None, :], x)  # empty MsgApps
        out = rng.random((S, G))
        x = np.where(out < bad / 2, r0[None, :] - 1, x)
        x = np.where(out > 1 - bad / 2, last[None, :] + 1, x)
        a = np.full((S, st), SENT, np.uint64)
        a[:, :G] = (x + shift).astype(np.uint64)
        return a

    peer = np.zeros((S, st), np.uint32)
    peer[:, :G] = rng.integers(0, 3, (S, G)) | (rng.integers(0, 1 << 20, (S, G)) << 2)
    full = (1 << S) - 1
    md = np.uint8 if S <= 8 else np.uint16
    top = int(np.iinfo(md).max)

    def mask(snap=False):
        """The snap bit wins over the others, so the dense shapes keep it sparse."""
        if density == "none":
            m = np.zeros(G, np.int64)
        elif density == "all" and not snap:
            m = np.full(G, top, np.int64)     # the bits at and above S too
        elif density == "last":
            m = np.zeros(G, np.int64)
            m[G - 1] = 1 if snap else full
        else:
            m = rng.integers(0, top + 1, G) * (rng.random(G) < (0.2 if snap else 0.6))
        return m.astype(md)

    state = dict(next=index_rows(1), peer=peer, committed=committed.astype(np.uint64),
                 first_index=(r0 + 1).astype(np.uint64), last_index=last.astype(np.uint64),
                 run_first=rf, run_term=rt, run_count=nr.astype(np.uint8),
                 snap_index=snap_index.astype(np.uint64))
    inp = dict(term=rng.integers(1, 1 << 40, G).astype(np.uint64))
    if "app" in kinds:
        inp["sent"] = mask()
        inp["index" if src == "index" else "next_before"] = index_rows(0 if src == "index" else 1)
    if "snap" in kinds:
        inp["snap"] = mask(snap=True)
    if "hb" in kinds:
        inp["hb_sent"] = mask()
        hc = rng.integers(0, 1 << 62, (S, st)).astype(np.uint64)
        inp["hb_commit"], inp["hb_ctx"] = hc, rng.integers(0, 1 << 32, G).astype(np.uint32)
    return state, inp


def model_arrays(recs, E):
    n = len(recs)
    a = {k: np.array([r[k] for r in recs], np.uint64) for k in om.FIELDS}
    el, et = np.zeros((E, n), np.uint64), np.zeros((E, n), np.uint64)
    for i, r in enumerate(recs):
        for j, (ln, t) in enumerate(r["ents"]):
            el[j, i], et[j, i] = ln, t
    return a, el, et


#        G    S  R   E  density   kinds                 src      max  cap     snap_term
CASES = [
    (1,    1,  1,  0, "all",    ("app",),              "index", 0, "full", False),
    (1,    3,  4,  4, "all",    ("app", "snap", "hb"), "next",  7, "cut",  True),
    (1,    16, 16, 1, "last",   ("app", "hb"),         "index", 1, "full", False),
    (63,   1,  4,  1, "random", ("app", "snap"),       "next",  0, "full", False),
    (63,   3,  16, 4, "all",    ("app", "snap", "hb"), "index", 7, "full", True),
    (63,   5,  1,  4, "random", ("app", "snap", "hb"), "next",  1, "cut",  False),
    (63,   16, 4,  0, "random", ("app", "hb"),         "index", 0, "full", False),
    (63,   5,  4,  1, "none",   ("app", "snap", "hb"), "index", 0, "full", False),
    (65,   1,  16, 4, "random", ("app", "snap", "hb"), "index", 0, "zero", False),
    (65,   3,  1,  1, "last",   ("app", "snap"),       "next",  7, "full", True),
    (65,   5,  4,  4, "all",    ("app", "snap", "hb"), "next",  0, "cut",  False),
    (65,   16, 16, 4, "random", ("app", "snap", "hb"), "next",  0, "full", True),
    (65,   5,  16, 0, "random", ("hb",),               "index", 0, "full", False),
    (65,   16, 1,  1, "all",    ("hb",),               "index", 0, "cut",  False),
    (65,   3,  4,  4, "random", ("snap",),             "index", 0, "full", True),
    (65,   5,  16, 1, "random", ("app",),              "index", 7, "full", False),
    (BIG,  1,  4,  4, "all",    ("app", "snap", "hb"), "index", 0, "full", False),
    (BIG,  3,  4,  4, "random", ("app", "snap", "hb"), "next",  7, "cut",  False),
    (BIG,  5,  16, 4, "random", ("app", "snap"),       "index", 1, "full", True),
    (BIG,  16, 1,  0, "random", ("app", "hb"),         "next",  0, "full", False),
    (BIG,  3,  1,  1, "all",    ("app",),              "next",  0, "cut",  False),
    (BIG,  5,  4,  0, "last",   ("app", "snap", "hb"), "index", 7, "full", False),
    (BIG,  16, 16, 1, "last",   ("app", "snap", "hb"), "next",  1, "zero", True),
    (BIG,  5,  16, 4, "none",   ("app", "snap", "hb"), "next",  0, "full", False),
    (BIG,  3,  16, 1, "random", ("hb",),               "index", 0, "full", False),
]


def test_chunk_size(eng):
    """CHUNK is the chunk the library is built with: the scratch grows by one
    offset and one count at every multiple of it."""
    L = eng._lib.lib()
    assert L.qe_outbox_scratch_bytes(CHUNK) + 12 == L.qe_outbox_scratch_bytes(CHUNK + 1)
    assert L.qe_outbox_scratch_bytes(1) == L.qe_outbox_scratch_bytes(CHUNK)


@pytest.mark.parametrize("G,S,R,E,density,kinds,src,max_entries,cap_mode,with_snap_term", CASES)
def test_outbox_matches_model(eng, G, S, R, E, density, kinds, src, max_entries, cap_mode,
                              with_snap_term):
    e = eng
    rng = np.random.default_rng(zlib.crc32(repr((G, S, R, E, density, kinds, src, max_entries)).encode()))
    state, inp = random_case(rng, G, S, R, density, kinds, src)
    st = G + 3
    if with_snap_term:
        inp["snap_term"] = rng.integers(1, 1 << 40, G).astype(np.uint64)
    # ---- the model ----
    flat = lambda d: {k: np.asarray(v).reshape(-1) for k, v in d.items()}  # noqa: E731
    mst = om.state(num_groups=G, group_offset=GOFF, num_slots=S, stride=st, log_runs=R,
                   **flat(state))
    recs, mstats = om.build(mst, om.inputs(max_entries=max_entries, **flat(inp)), E)
    count = len(recs)
    cap = {"full": count + 5, "cut": max(count - 1, 0), "zero": 0}[cap_mode]
    n = min(count, cap)
    if density == "none":
        assert count == 0
    elif density == "last":
        assert 0 < count <= S
    # ---- the device ----
    ps = e.ProgressState(G, S, 1, R, DEV, group_offset=GOFF, stride=st, extras=("snap_index",))
    for k, a in state.items():
        put(getattr(ps, k), a)
    before = {k: getattr(ps, k).clone() for k in ps.ARRAYS if getattr(ps, k) is not None}
    ob = e.Outbox(ps, cap, E)
    for k in ob.ARRAYS:
        t = getattr(ob, k)
        if t is not None:
            t.view(torch.uint8).fill_(SENT & 0xFF)
    d = {k: dev(v) for k, v in inp.items()}
    stats = e.stats_buffer(DEV)
    e.outbox(ps, d["term"], ob, sent=d.get("sent"), snap=d.get("snap"), index=d.get("index"),
             next_before=d.get("next_before"), hb_sent=d.get("hb_sent"),
             hb_commit=d.get("hb_commit"), hb_ctx=d.get("hb_ctx"), snap_term=d.get("snap_term"),
             max_entries=max_entries, stats=stats)
    folded = host(e.stats_reduce(stats))
    torch.cuda.synchronize()
    # ---- nothing of the resident state moved ----
    for k, t in before.items():
        assert torch.equal(getattr(ps, k), t), k + " was written"
    # ---- count, the records, the untouched rest ----
    assert int(host(ob.count)[0]) == count
    want, el, et = model_arrays(recs[:n], E)
    eq = np.testing.assert_array_equal
    width = max(1, cap)
    for k in om.FIELDS:
        got = host(getattr(ob, k))
        eq(got[:n], want[k].astype(got.dtype), err_msg=k)
        rest = got[n:].view(np.uint8)
        assert (rest == SENT & 0xFF).all(), k + ": written past min(count, capacity)"
    if E:
        gl, gt = host(ob.ent_len).reshape(E, width), host(ob.ent_term).reshape(E, width)
        eq(gl[:, :n], el.astype(np.uint32), err_msg="ent_len")
        eq(gt[:, :n], et, err_msg="ent_term")
        assert (gl[:, n:].view(np.uint8) == SENT & 0xFF).all(), "ent_len past the prefix"
        assert (gt[:, n:].view(np.uint8) == SENT & 0xFF).all(), "ent_term past the prefix"
    # ---- the statistics count every record, past capacity too ----
    for i in range(16):
        assert int(folded[i]) == mstats.get(i, 0), ("stat", i)


def walk_groups():
    """The smallest batch at which a fill block takes a second chunk: with
    statistics the fill grid is capped at 8 blocks per CU, so one chunk more
    than that, and the ragged 65 groups of BIG."""
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    return (8 * cus + 1) * CHUNK + 65


class DeviceRandom:
    """Seeded random rows of G groups, generated on the device."""

    def __init__(self, G, seed):
        self.G, self.gen = G, torch.Generator(device=DEV).manual_seed(seed)

    def ints(self, lo, hi, dtype=torch.int64):
        return torch.randint(lo, hi, (self.G,), generator=self.gen, device=DEV).to(dtype)

    def hit(self, p):
        """True for about p of the groups."""
        return torch.rand(self.G, generator=self.gen, device=DEV) < p


def same_list(a, b, runs, width):
    """-> the common count of two record lists, after comparing count and
    every record array up to it on the device; the rows named in `runs` are
    [E][capacity]."""
    assert torch.equal(a.count, b.count), "count"
    n = int(a.count.item())
    assert 0 < n <= a.capacity == b.capacity
    for k in a.ARRAYS:
        x, y = getattr(a, k), getattr(b, k)
        if k == "count" or x is None:
            assert k == "count" or y is None
            continue
        if k in runs:
            x, y = x.view(width, -1)[:, :n], y.view(width, -1)[:, :n]
        else:
            x, y = x[:n], y[:n]
        assert torch.equal(x, y), k
    return n


def test_fill_blocks_walk(eng):
    """A batch of one chunk more than the capped fill grid has blocks: with
    statistics a block takes a second chunk.  The list of that call against the
    list of the call without statistics (a block per chunk, what the model
    tests pin), and the counters the list alone determines."""
    e, L = eng, eng._lib
    G, S, R, E = walk_groups(), 1, 1, 1
    rnd = DeviceRandom(G, 0x0B0C)
    ps = e.ProgressState(G, S, 1, R, DEV, group_offset=GOFF, extras=("snap_index",))
    ps.run_first[:G], ps.run_term[:G], ps.run_count[:] = 5, 3, 1
    ps.last_index.copy_(5 + rnd.ints(0, 12))
    ps.committed.fill_(5)
    ps.snap_index.fill_(4)
    index = torch.zeros(S * ps.stride, dtype=torch.int64, device=DEV)
    index[:G] = 5 + rnd.ints(0, 13)  # a few past last_index: QE_OMSG_BAD
    hb_commit = torch.zeros(S * ps.stride, dtype=torch.int64, device=DEV)
    hb_commit[:G] = rnd.ints(0, 1 << 40)
    sent, snap, hb = (rnd.hit(p).to(torch.uint8) for p in (0.01, 0.003, 0.01))
    term, ctx = rnd.ints(1, 1 << 40), rnd.ints(0, 1 << 31, torch.int32)
    cap = int(((sent | snap | hb) & 1).sum().item()) + 5  # one slot: a record per group at most
    lists = []
    for stats in (None, e.stats_buffer(DEV)):
        ob = e.Outbox(ps, cap, E)
        e.outbox(ps, term, ob, sent=sent, snap=snap, index=index, hb_sent=hb, hb_commit=hb_commit,
                 hb_ctx=ctx, stats=stats)
        lists.append(ob)
    n = same_list(lists[0], lists[1], ("ent_len", "ent_term"), E)
    folded = e.stats_reduce(stats)
    t = lists[0].type[:n]
    per_type = {L.QE_STAT_OUTBOX_APP: L.QE_OMSG_APP, L.QE_STAT_OUTBOX_SNAP: L.QE_OMSG_SNAP,
                L.QE_STAT_OUTBOX_HEARTBEAT: L.QE_OMSG_HEARTBEAT, L.QE_STAT_OUTBOX_BAD: L.QE_OMSG_BAD}
    for stat, ty in per_type.items():
        assert int(folded[stat].item()) == int((t == ty).sum().item()) > 0, ("stat", stat)
    assert sum(int(folded[stat].item()) for stat in per_type) == n  # the record count
