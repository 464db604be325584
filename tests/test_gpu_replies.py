"""qe_replies on the device against tests/replies_model.py on random inputs:
every record array up to min(count, capacity), count and the statistics; the
outputs are prefilled with the sentinel of tests/test_gpu_cluster.py and
everything past the written prefix must keep it; the resident state and every
input row must be byte-identical before and after.

The shapes: G = 1 (one lane), 63 (a ragged single tile), 65 (a ragged second
tile) and 3 chunks + 65 (three scan chunks, the chunk being the 4096 groups the
library is built with); S = 1, 3, 5 (8-bit masks) and 16 (16-bit); every family
alone, all four, V + T; stride = G + 3; group_offset 2^33; indices and terms
straddling 2^32.  The random result codes run over the whole code range (the
codes that yield nothing and the refused ones included) and a few percent of
the `from` rows name no slot."""
import zlib

import numpy as np
import pytest
import torch

from tests import replies_model as rm
from tests.test_gpu_outbox import (BIG, CHUNK, DEV, GOFF, SENT, DeviceRandom, dev, eng,  # noqa: F401
                                   host, same_list, walk_groups)

pytestmark = pytest.mark.gpu
CODES = {"F": [0, 1, 2, 3, 4, 5, 6, 7, 15, 16, 17, 18, 19, 20, 255],
         "S": [0, 1, 2, 3, 4, 5, 6, 16, 17, 18, 255],
         "V": [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 16, 200]}
SENDS = {"F": [2, 3, 4, 5, 6], "S": [2, 3, 4, 5], "V": [3, 4, 8, 9]}


def random_case(rng, G, S, fams, density, with_f_ctx, bad=0.04):
    """-> (last_index, the inputs) as numpy arrays."""
    md = np.uint8 if S <= 8 else np.uint16
    top, full = int(np.iinfo(md).max), (1 << S) - 1
    near = lambda: ((1 << 32) - 40 + rng.integers(0, 80, G)).astype(np.uint64)  # noqa: E731

    def results(fam):
        quiet = [c for c in CODES[fam] if c not in SENDS[fam]]
        if density == "all":
            r = rng.choice(SENDS[fam], G)
        elif density == "random":
            r = rng.choice(CODES[fam], G)
        else:
            r = rng.choice(quiet, G)
            if density == "last":
                r[G - 1] = rng.choice(SENDS[fam])
        return r.astype(np.uint8)

    def slots():
        f = rng.integers(0, S, G)
        out = rng.random(G)
        f = np.where(out < bad / 2, S, f)
        f = np.where(out > 1 - bad / 2, 0xFF, f)
        return f.astype(np.uint8)

    def mask():
        if density == "all":
            m = np.full(G, top, np.int64)  # the bits at and above S too
        elif density == "random":
            m = rng.integers(0, top + 1, G) * (rng.random(G) < 0.5)
        else:
            m = np.full(G, top & ~full, np.int64)  # only bits that name no slot
            if density == "last":
                m[G - 1] = top
        return m.astype(md)

    inp = dict(term=near())
    if "F" in fams:
        inp.update(f_result=results("F"), f_from=slots(), f_resp_index=near(),
                   f_reject_hint=near(), f_resp_log_term=rng.integers(1, 1 << 40, G).astype(np.uint64))
        if with_f_ctx:
            inp["f_ctx"] = rng.integers(0, 1 << 32, G).astype(np.uint32)
    if "S" in fams:
        inp.update(s_result=results("S"), s_from=slots(), s_resp_index=near())
    if "V" in fams:
        vt = np.where(rng.random(G) < 0.7, rng.integers(1, 3, G), rng.integers(0, 8, G))
        vt = np.where(rng.random(G) < 0.3, 6, vt)  # MsgTimeoutNow: FORCE on a campaign
        req = rng.integers(0, top + 1, G).astype(md)  # read for a campaign alone
        inp.update(v_result=results("V"), v_type=vt.astype(np.uint8), v_from=slots(),
                   v_resp_term=near(), v_req_log_term=near(), v_req_to=req)
    if "T" in fams:
        inp["timeout_now"] = mask()
    return near(), inp


#        G    S   fams    density   cap     ctx    flags  f_ctx
CASES = [
    (1,   1,  "FSVT", "all",    "full", True,  True,  True),
    (1,   3,  "F",    "all",    "cut",  True,  True,  False),
    (1,   16, "VT",   "last",   "full", False, False, False),
    (63,  1,  "S",    "random", "full", True,  True,  False),
    (63,  3,  "FSVT", "all",    "full", True,  True,  True),
    (63,  5,  "V",    "random", "cut",  True,  False, False),
    (63,  16, "T",    "random", "full", False, True,  False),
    (63,  5,  "FSVT", "none",   "full", True,  True,  True),
    (65,  1,  "FSVT", "random", "zero", True,  True,  True),
    (65,  3,  "VT",   "last",   "full", True,  True,  False),
    (65,  5,  "FSVT", "all",    "cut",  True,  True,  False),
    (65,  16, "FSVT", "random", "full", True,  True,  True),
    (65,  5,  "T",    "random", "full", True,  True,  False),
    (65,  16, "F",    "all",    "cut",  False, False, True),
    (65,  3,  "S",    "random", "full", True,  True,  False),
    (65,  5,  "V",    "random", "full", True,  True,  False),
    (BIG, 1,  "FSVT", "all",    "full", True,  True,  True),
    (BIG, 3,  "FSVT", "random", "cut",  True,  True,  True),
    (BIG, 5,  "V",    "random", "full", True,  True,  False),
    (BIG, 16, "VT",   "random", "full", True,  True,  False),
    (BIG, 3,  "F",    "all",    "cut",  True,  False, False),
    (BIG, 5,  "FSVT", "last",   "full", True,  True,  True),
    (BIG, 16, "FSVT", "last",   "zero", False, False, False),
    (BIG, 5,  "FSVT", "none",   "full", True,  True,  False),
    (BIG, 3,  "T",    "random", "full", True,  True,  False),
]


class Rows:
    """The device rows of one family under the names engine.replies reads."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def test_chunk_size(eng):  # noqa: F811
    """CHUNK is the chunk the library is built with (qe_outbox's)."""
    L = eng._lib.lib()
    assert L.qe_replies_scratch_bytes(CHUNK) + 12 == L.qe_replies_scratch_bytes(CHUNK + 1)
    assert L.qe_replies_scratch_bytes(1) == L.qe_replies_scratch_bytes(CHUNK)


@pytest.mark.parametrize("G,S,fams,density,cap_mode,with_ctx,with_flags,with_f_ctx", CASES)
def test_replies_match_model(eng, G, S, fams, density, cap_mode, with_ctx, with_flags,  # noqa: F811
                             with_f_ctx):
    e = eng
    rng = np.random.default_rng(zlib.crc32(repr((G, S, fams, density, with_f_ctx)).encode()))
    last, inp = random_case(rng, G, S, fams, density, with_f_ctx)
    st = G + 3
    # ---- the model ----
    recs, mstats = rm.build(rm.state(num_groups=G, group_offset=GOFF, num_slots=S, stride=st,
                                     last_index=last), rm.inputs(**inp))
    count = len(recs)
    cap = {"full": count + 5, "cut": max(count - 1, 0), "zero": 0}[cap_mode]
    n = min(count, cap)
    if density == "none":
        assert count == 0
    elif density == "last":
        assert 0 < count <= 3 + 2 * S
    elif density == "all":
        assert count >= G
    # ---- the device ----
    ps = e.ProgressState(G, S, 1, 1, DEV, group_offset=GOFF, stride=st)
    ps.last_index.copy_(dev(last))
    before = {k: getattr(ps, k).clone() for k in ps.ARRAYS if getattr(ps, k) is not None}
    rp = e.Replies(ps, cap, ctx=with_ctx, flags=with_flags)
    for k in rp.ARRAYS:
        t = getattr(rp, k)
        if t is not None:
            t.view(torch.uint8).fill_(SENT & 0xFF)
    d = {k: dev(v) for k, v in inp.items()}
    d0 = {k: t.clone() for k, t in d.items()}
    g = d.get
    follow = (Rows(from_=g("f_from")), Rows(result=g("f_result"), resp_index=g("f_resp_index"),
                                            reject_hint=g("f_reject_hint"),
                                            resp_log_term=g("f_resp_log_term")))
    snap = (Rows(from_=g("s_from")), Rows(result=g("s_result"), resp_index=g("s_resp_index")))
    vote = (Rows(type=g("v_type"), from_=g("v_from")),
            Rows(result=g("v_result"), resp_term=g("v_resp_term"),
                 req_log_term=g("v_req_log_term"), req_to=g("v_req_to")))
    stats = e.stats_buffer(DEV)
    e.replies(ps, d["term"], rp, follow=follow if "F" in fams else None,
              snap=snap if "S" in fams else None, vote=vote if "V" in fams else None,
              timeout_now=g("timeout_now"), f_ctx=g("f_ctx"), stats=stats)
    folded = host(e.stats_reduce(stats))
    torch.cuda.synchronize()
    # ---- nothing of the resident state or of the inputs moved ----
    for k, t in before.items():
        assert torch.equal(getattr(ps, k), t), k + " was written"
    for k, t in d0.items():
        assert torch.equal(d[k], t), "input " + k + " was written"
    # ---- count, the records, the untouched rest ----
    assert int(host(rp.count)[0]) == count
    for k in rm.FIELDS:
        t = getattr(rp, k)
        if t is None:
            assert (k == "ctx" and not with_ctx) or (k == "flags" and not with_flags)
            continue
        got = host(t)
        want = np.array([r[k] for r in recs[:n]], np.uint64)
        np.testing.assert_array_equal(got[:n], want.astype(got.dtype), err_msg=k)
        assert (got[n:].view(np.uint8) == SENT & 0xFF).all(), \
            k + ": written past min(count, capacity)"
    # ---- the statistics count every record, past capacity too ----
    for i in range(16):
        assert int(folded[i]) == mstats.get(i, 0), ("stat", i)


def test_fill_blocks_walk(eng):  # noqa: F811
    """test_fill_blocks_walk of tests/test_gpu_outbox.py for qe_replies: every
    family, sparse, on one chunk more than the capped fill grid has blocks."""
    e, L = eng, eng._lib
    G, S = walk_groups(), 1
    rnd = DeviceRandom(G, 0x0E11)
    u8 = torch.uint8
    zero = torch.zeros(G, dtype=u8, device=DEV)
    ps = e.ProgressState(G, S, 1, 1, DEV, group_offset=GOFF)
    ps.last_index.copy_(rnd.ints(1, 1 << 40))
    slots = lambda: rnd.hit(0.05).to(u8)  # noqa: E731  (slot 0, a few that name no slot)
    f_result = torch.where(rnd.hit(0.01), 2 + rnd.ints(0, 5, u8), zero)
    s_result = torch.where(rnd.hit(0.005), 2 + rnd.ints(0, 4, u8), zero)
    codes = torch.tensor([3, 4, 8, 9], dtype=u8, device=DEV)
    v_result = torch.where(rnd.hit(0.01), codes[rnd.ints(0, 4)], zero)
    v_type = torch.where(rnd.hit(0.2), torch.full_like(zero, 6), rnd.ints(1, 3, u8))
    req_to, tn = rnd.ints(0, 256, u8), rnd.hit(0.005).to(u8)
    follow = (Rows(from_=slots()), Rows(result=f_result, resp_index=rnd.ints(1, 1 << 40),
                                        reject_hint=rnd.ints(1, 1 << 40),
                                        resp_log_term=rnd.ints(1, 1 << 40)))
    snap = (Rows(from_=slots()), Rows(result=s_result, resp_index=rnd.ints(1, 1 << 40)))
    vote = (Rows(type=v_type, from_=slots()),
            Rows(result=v_result, resp_term=rnd.ints(1, 1 << 40),
                 req_log_term=rnd.ints(1, 1 << 40), req_to=req_to))
    term, f_ctx = rnd.ints(1, 1 << 40), rnd.ints(0, 1 << 31, torch.int32)
    sends = ((f_result - 2 <= 4).sum() + (s_result - 2 <= 3).sum() + (v_result - 3 <= 1).sum() +
             ((v_result - 8 <= 1) & ((req_to & 1) != 0)).sum() + tn.sum())  # (u8: 0 - 2 wraps)
    cap = int(sends.item()) + 5
    lists = []
    for stats in (None, e.stats_buffer(DEV)):
        rp = e.Replies(ps, cap)
        e.replies(ps, term, rp, follow=follow, snap=snap, vote=vote, timeout_now=tn, f_ctx=f_ctx,
                  stats=stats)
        lists.append(rp)
    n = same_list(lists[0], lists[1], (), 0)
    folded = e.stats_reduce(stats)
    t = lists[0].type[:n]
    per_type = {L.QE_STAT_REPLY_APP_RESP: (L.QE_IMSG_APP_RESP, L.QE_IMSG_APP_RESP_REJECT),
                L.QE_STAT_REPLY_HEARTBEAT_RESP: (L.QE_IMSG_HEARTBEAT_RESP,),
                L.QE_STAT_REPLY_VOTE_RESP: (L.QE_IMSG_VOTE_RESP, L.QE_IMSG_PREVOTE_RESP),
                L.QE_STAT_REPLY_VOTE_REQ: (L.QE_IMSG_VOTE, L.QE_IMSG_PREVOTE),
                L.QE_STAT_REPLY_TIMEOUT_NOW: (L.QE_IMSG_TIMEOUT_NOW,),
                L.QE_STAT_REPLY_BAD: (L.QE_RMSG_BAD,)}
    for stat, types in per_type.items():
        want = sum(int((t == ty).sum().item()) for ty in types)
        assert int(folded[stat].item()) == want > 0, ("stat", stat)
    assert sum(int(folded[stat].item()) for stat in per_type) == n  # the record count
