"""qe_carry on the device against tests/carry_model.py, bit for bit, on the
cases the model's own test shares (carry_model.cases()): through the raw C call
with every output array compared whole, sentinel-filled tails included, and
through engine.carry into an Inbox."""
import ctypes as C

import numpy as np
import pytest
import torch

from etcd_amd import _lib
from tests import carry_model as m
from tests.test_gpu_progress import DEV

pytestmark = pytest.mark.gpu
CASES = m.cases()
BY_NAME = {c.name: c for c in CASES}
SENT = {np.dtype(np.uint64): 0xEEEEEEEEEEEEEEEE, np.dtype(np.uint32): 0xEEEEEEEE,
        np.dtype(np.uint8): 0xEE}
SIGNED = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32,
          np.dtype(np.uint16): np.int16, np.dtype(np.uint8): np.uint8}
OUT = dict(m.FIELDS, **m.ENTS)


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from etcd_amd import engine
    return engine


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(SIGNED[a.dtype]).reshape(-1).copy()).to(DEV)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def sentinel(size, dtype):
    return np.full(max(1, size), SENT[np.dtype(dtype)], dtype)


def raw(eng, c, out_cap, base=0, pitch=None, stats=None):
    """The C call on case c -> (status, every output array as numpy, whole; the folded
    statistics or None).  Every output starts sentinel-filled."""
    st, src, cap = c.st, c.src, len(c.src["group"])
    pitch = out_cap if pitch is None else pitch
    E_in = 0 if src.get("ent_len") is None else len(src["ent_len"])
    d = {k: dev(v) for k, v in src.items() if k != "count"}
    d["count"] = dev(np.array([src["count"]], np.uint64))
    d["drop"], d["cut"] = dev(c.drop), dev(c.cut)
    pg, pf = dev(c.peer_group), dev(c.peer_from)
    o = {k: dev(sentinel(c.E_out * pitch if k in m.ENTS else out_cap, t)) for k, t in OUT.items()}
    if not c.E_out:
        o["ent_len"] = o["ent_term"] = None
    o["disposition"], o["remote"] = dev(sentinel(cap, np.uint8)), dev(sentinel(cap, np.uint32))
    o["counts"] = dev(sentinel(2, np.uint64))
    L = _lib.lib()
    scratch = torch.empty(L.qe_carry_scratch_bytes(cap) // 8 + 1, dtype=torch.int64, device=DEV)
    sb = eng.stats_buffer(DEV) if stats else None
    p = _lib.QeProgress(num_groups=st.num_groups, group_offset=st.group_offset,
                        num_slots=st.num_slots, stride=st.stride)
    pe = _lib.QePeers(ptr(pg), ptr(pf))
    i = _lib.QeCarryIn(cap, ptr(d["count"]), E_in, _lib.QE_CARRY_SNAP_STATUS if c.snap_status else 0,
                       *[ptr(d.get(k)) for k in ("group", "to", "type", "term", "index", "log_term",
                                                 "commit", "hint", "ctx", "mflags", "ent_len",
                                                 "ent_term", "drop", "cut")], c.ignore, 0)
    oo = _lib.QeCarryOut(out_cap, base, pitch, c.E_out, 0,
                         *[ptr(o[k]) for k in ("group", "from", "type", "term", "index", "log_term",
                                               "commit", "hint", "ctx", "mflags", "ent_len",
                                               "ent_term", "src")],
                         C.c_void_p(o["counts"].data_ptr()), ptr(o["disposition"]), ptr(o["remote"]),
                         C.c_void_p(o["counts"].data_ptr() + 8))
    status = L.qe_carry(C.byref(p), C.byref(pe), C.byref(i), C.byref(oo), ptr(scratch), ptr(sb),
                        C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    torch.cuda.synchronize()
    kinds = dict(OUT, disposition=np.uint8, remote=np.uint32, counts=np.uint64)
    got = {k: None if t is None else t.cpu().numpy().view(kinds[k]) for k, t in o.items()}
    folded = eng.stats_reduce(sb).cpu().numpy().view(np.uint64) if stats else None
    return status, got, folded


def expected(c, out_cap, base, pitch):
    w, cap = c.want, len(c.src["group"])
    exp = {k: sentinel(c.E_out * pitch if k in m.ENTS else out_cap, t) for k, t in OUT.items()}
    if not c.E_out:
        exp["ent_len"] = exp["ent_term"] = None
    m.place(w, exp, base, out_cap, pitch)
    exp["disposition"], exp["remote"] = sentinel(cap, np.uint8), sentinel(cap, np.uint32)
    exp["disposition"][:w.n] = w.disposition      # not touched at or past n
    exp["remote"][:len(w.remote)] = w.remote
    exp["counts"] = np.array([w.count, len(w.remote)], np.uint64)
    return exp


def check(c, got, exp, folded):
    for k, e in exp.items():
        if e is None:
            assert got[k] is None
        else:
            assert np.array_equal(got[k], e), (c.name, k, np.flatnonzero(got[k] != e)[:8])
    if folded is not None:
        assert np.array_equal(folded, c.want.stats), (c.name, folded, c.want.stats)


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_raw_call_matches_model_whole_arrays(eng, name):
    """Room for every record and five more: the tails keep their sentinels."""
    c = BY_NAME[name]
    out_cap = c.want.count + 5
    status, got, folded = raw(eng, c, out_cap, stats=c.stats)
    assert status == _lib.QE_OK
    check(c, got, expected(c, out_cap, 0, out_cap), folded)


def test_base_and_a_pitch_above_capacity(eng):
    c = BY_NAME["n4161-outbox"]
    assert c.E_out > 0
    base, out_cap = 77, 77 + c.want.count + 9
    status, got, folded = raw(eng, c, out_cap, base=base, pitch=out_cap + 13, stats=True)
    assert status == _lib.QE_OK
    check(c, got, expected(c, out_cap, base, out_cap + 13), folded)
    assert (got["group"][:base] == SENT[np.dtype(np.uint64)]).all()  # nothing below base


@pytest.mark.parametrize("name", ["n65-outbox", "n8193-replies", "n4161-outbox"])
def test_truncation_room_for_half(eng, name):
    """*count and the statistics are still the full numbers."""
    c = BY_NAME[name]
    base = 3
    out_cap = base + c.want.count // 2
    status, got, folded = raw(eng, c, out_cap, base=base, stats=True)
    assert status == _lib.QE_OK and got["counts"][0] == c.want.count > out_cap - base
    check(c, got, expected(c, out_cap, base, out_cap), folded)
    # no room at all: base == capacity
    status, got, _ = raw(eng, c, base, base=base)
    assert status == _lib.QE_OK
    check(c, got, expected(c, base, base, base), None)


def test_records_behind_count_are_ignored(eng):
    c = BY_NAME["count-below-capacity"]
    cap = len(c.src["group"])
    assert c.want.n == c.src["count"] < cap and np.isin(c.src["type"][c.want.n:], m.CARRIABLE).any()
    _, got, _ = raw(eng, c, c.want.count + 5)
    assert (got["disposition"][c.want.n:] == 0xEE).all()
    c = BY_NAME["count-above-capacity"]
    assert c.src["count"] > len(c.src["group"]) == c.want.n


def test_two_runs_are_identical(eng):
    c = BY_NAME["n8193-outbox"]
    a = raw(eng, c, c.want.count, stats=True)
    b = raw(eng, c, c.want.count, stats=True)
    assert all(np.array_equal(a[1][k], b[1][k]) for k in a[1] if a[1][k] is not None)
    assert np.array_equal(a[2], b[2])


def load_engine(eng, c, room):
    st, src, cap = c.st, c.src, len(c.src["group"])
    E_in = 0 if src.get("ent_len") is None else len(src["ent_len"])
    ps = eng.ProgressState(st.num_groups, st.num_slots, 1, 1, DEV, group_offset=st.group_offset,
                           stride=st.stride)
    peers = eng.Peers(ps).load_host(peer_group=c.peer_group, peer_from=c.peer_from)
    if c.form == "outbox":
        s = eng.Outbox(ps, cap, E_in)
        s.load_host(**{k: v for k, v in src.items() if k != "count"})
    else:
        s = eng.Replies(ps, cap)
        s.load_host(**{("flags" if k == "mflags" else k): v for k, v in src.items() if k != "count"})
    s.count.fill_(int(src["count"]))
    ib = eng.Inbox(ps, room, c.E_out)
    return ps, peers, s, ib


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_engine_matches_model(eng, name):
    """engine.carry from an Outbox / a Replies as it stands into an Inbox that already holds
    three records: they stay, the carried ones follow, the ent rows at the new pitch."""
    c, w = BY_NAME[name], BY_NAME[name].want
    ps, peers, s, ib = load_engine(eng, c, w.count + 3)
    E = c.E_out
    pre = dict(group=np.array([5, 6, 7], np.uint64), type=np.array([1, 3, 4], np.uint8),
               index=np.array([1 << 63, 2, 3], np.uint64))
    pre_ents = {"ent_len": np.arange(3 * E, dtype=np.uint32).reshape(E, 3) + 9,
                "ent_term": np.arange(3 * E, dtype=np.uint64).reshape(E, 3) + 99}
    ib.load_host(**pre, **(pre_ents if E else {}))
    sb = eng.stats_buffer(DEV) if c.stats else None
    res = eng.carry(ps, peers, s, ib, drop=dev(c.drop) if len(c.drop) else None, cut=c.cut,
                    ignore=c.ignore, snap_status=c.snap_status, stats=sb)
    assert (res.n, res.count, res.remote_count) == (w.n, w.count, len(w.remote))
    assert ib.n == 3 + w.count
    disp, remote = res.host()
    assert np.array_equal(disp, w.disposition) and np.array_equal(remote, w.remote)
    assert np.array_equal(res.src.cpu().numpy().view(np.uint32), w.local["src"])
    host = ib.host()
    for k in ib.RECORD:
        f = {"from_": "from", "flags": "mflags"}.get(k, k)
        head = pre.get(k, np.zeros(3, w.local[f].dtype))
        assert np.array_equal(host[k][:ib.n], np.concatenate([head, w.local[f]])), (name, k)
    for k in m.ENTS if E else ():
        rows = host[k][:E * ib.n].reshape(E, ib.n)
        assert np.array_equal(rows, np.concatenate([pre_ents[k], w.local[k]], axis=1)), (name, k)
    if sb is not None:
        assert np.array_equal(eng.stats_reduce(sb).cpu().numpy().view(np.uint64), w.stats)


def test_engine_refuses_what_does_not_fit(eng):
    c = BY_NAME["n65-replies"]
    ps, peers, s, ib = load_engine(eng, c, c.want.count - 1)
    with pytest.raises(ValueError):
        eng.carry(ps, peers, s, ib, drop=c.drop, cut=c.cut, ignore=c.ignore)
    assert ib.n == 0
    with pytest.raises(ValueError):
        eng.carry(ps, peers, s, ib, after=1)


def test_peers_clusters_is_the_static_layout(eng):
    ps = eng.ProgressState(10, 4, 1, 1, DEV, group_offset=1 << 40)
    h = eng.Peers.clusters(ps, 3).host()
    pg, pf = h["peer_group"].reshape(4, ps.stride), h["peer_from"].reshape(4, ps.stride)
    g = np.arange(9)
    for s in range(3):
        assert np.array_equal(pg[s, :9], ((1 << 40) + g - g % 3 + s).astype(np.uint64))
        assert np.array_equal(pf[s, :9], (g % 3).astype(np.uint8))
    assert pg[0, 9] == (1 << 40) + 9 and pf[0, 9] == 0          # the ragged last cluster
    assert (pg[1:, 9] == _lib.QE_PEER_NONE).all() and (pg[3] == _lib.QE_PEER_NONE).all()
