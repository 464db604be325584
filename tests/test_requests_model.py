"""tests/requests_model.py pinned to the reference: its tests of proposal
forwarding, ReadIndex forwarding and leadership transfer from a follower, and
the arms of stepCandidate / stepFollower, transcribed as data with file:line
provenance in tests/golden/request_tables.json; two negative controls that must
fail; and the order-free form the kernels use (stop by min) held against the
sequential loop on random lists.  Needs no GPU and no library."""
import json
import os
import random

import pytest

from tests import requests_model as qm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "request_tables.json")
with open(GOLDEN) as fh:
    TABLES = json.load(fh)
CASES = {c["name"]: c for c in TABLES["cases"]}
TYPE = {"MsgProp": qm.PROP, "MsgReadIndex": qm.READ_INDEX, "MsgReadIndexResp": qm.READ_INDEX_RESP,
        "MsgTransferLeader": qm.TRANSFER_LEADER}
STATE = {"follower": qm.ST_FOLLOWER, "candidate": qm.ST_CANDIDATE, "leader": qm.ST_LEADER,
         "pre_candidate": qm.ST_PRE_CANDIDATE}
DISP = {v: k for k, v in qm.QD_NAMES.items()}
KIND = {"FWD": qm.QO_FWD, "READ_STATE": qm.QO_READ_STATE, "PROP_DROPPED": qm.QO_PROP_DROPPED}
GROUP = 5  # any group of the batch


def slot(node_id):
    return qm.NONE if node_id == 0 else node_id - 1


def node_id(s):
    return 0 if s == qm.NONE else s + 1


def run_case(c, **switches):
    """-> (what the model gives, what the table wants), each as (disposition,
    the emitted record with ids, the row)."""
    n, m = c["node"], c["msg"]
    st = qm.state(num_groups=8, num_slots=3, term=[n["term"]] * 8, state=[STATE[n["state"]]] * 8,
                  lead=[slot(n["lead"])] * 8, self_slot=[slot(n["id"])] * 8)
    r = qm.rec(GROUP, TYPE[m["type"]], slot(m["from"]), m["term"], m["index"], m["key"],
               m["entries"] if m["type"] == "MsgProp" else 0)
    out = qm.route(st, [r], no_forward=c["no_forward"], **switches)
    got_out = None
    if out.records:
        (o,) = out.records
        assert (o["group"], o["src"]) == (GROUP, 0)
        got_out = dict(kind=o["kind"], type=o["type"], to=node_id(o["to"]), term=o["term"],
                       index=o["index"], key=o["key"])
        got_out["from"] = node_id(o["frm"])
    got_row = None
    if out.p:
        got_row = dict(family="proposal", num_entries=out.p[GROUP]["num_entries"])
    if out.r:
        ((s, g),) = out.r
        assert g == GROUP and out.r[(s, g)]["type"] == qm.MSG_TRANSFER_LEADER
        got_row = dict(family="peer", slot_id=node_id(s))
    w = c["want"]
    want_out = None
    if w["out"] is not None:
        want_out = dict(w["out"], kind=KIND[w["out"]["kind"]], type=TYPE[w["out"]["type"]])
    return (out.disposition[0], got_out, got_row), (DISP[w["disposition"]], want_out, w["row"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_case(name):
    got, want = run_case(CASES[name])
    assert got == want


def test_the_tables_cover_what_the_reference_tests_check():
    names = " ".join(CASES)
    for needle in ("ProposalByProxy", "DisableProposalForwarding", "NodeReadIndexToOldLeader",
                   "LeaderTransferToUpToDateNodeFromFollower", "stepCandidate drops",
                   "MsgReadIndexResp becomes"):
        assert needle in names, needle
    # every field of the four forwarded MsgReadIndex of TestNodeReadIndexToOldLeader
    fw = [CASES[n]["want"]["out"] for n in CASES if n.startswith("NodeReadIndexToOldLeader")]
    assert sorted((o["from"], o["to"], o["term"]) for o in fw) == \
        [(2, 1, 0), (2, 3, 0), (3, 1, 0), (3, 3, 0)]


@pytest.mark.parametrize("control", TABLES["negative_controls"], ids=lambda c: c["model_switch"])
def test_negative_control_fails(control):
    c = CASES[control["must_fail"]]
    got, want = run_case(c)
    assert got == want
    got, want = run_case(c, **{control["model_switch"]: True})
    assert got != want


def test_stepdown_and_its_read_state():
    """Rule 2: a higher term closes the group in any state; a READ_INDEX_RESP
    also yields its ReadState, a TRANSFER_LEADER yields nothing."""
    for role in (qm.ST_FOLLOWER, qm.ST_CANDIDATE, qm.ST_LEADER, qm.ST_PRE_CANDIDATE):
        st = qm.state(num_groups=2, num_slots=3, term=[4, 4], state=[role] * 2, lead=[1, 1],
                      self_slot=[0, 0])
        out = qm.route(st, [qm.rec(0, qm.READ_INDEX_RESP, 1, term=5, index=9, key=77),
                            qm.rec(1, qm.TRANSFER_LEADER, 2, term=6),
                            qm.rec(1, qm.READ_INDEX, key=3),
                            qm.rec(0, qm.READ_INDEX_RESP, 1, term=3, index=9, key=78),
                            qm.rec(1, qm.PROP, term=0, num_entries=0)])
        assert out.disposition == [qm.STEPDOWN, qm.STEPDOWN, qm.DEFERRED, qm.DEFERRED, qm.BAD]
        assert out.v[0] == dict(type=qm.VMSG_VOTE_RESP, frm=1, term=5, index=0, log_term=0,
                                flags=qm.VMF_REJECT, src=0)
        assert out.v[1]["term"] == 6 and out.v[1]["frm"] == 2
        assert out.records == [dict(group=0, kind=qm.QO_READ_STATE, type=qm.READ_INDEX_RESP,
                                    to=qm.NONE, frm=qm.NONE, term=0, index=9, key=77, src=0)]


def test_lower_term_and_ref_panic():
    st = qm.state(num_groups=1, num_slots=3, term=[4], state=[qm.ST_FOLLOWER], lead=[1],
                  self_slot=[0])
    out = qm.route(st, [qm.rec(0, qm.READ_INDEX_RESP, 1, term=3), qm.rec(0, qm.TRANSFER_LEADER, 2, 4),
                        qm.rec(0, qm.TRANSFER_LEADER, 2, 0)])
    assert out.disposition == [qm.DROP_LOWER_TERM, qm.REF_PANIC, qm.FORWARDED]
    assert out.stats[qm.STAT_VIOLATIONS] == 1
    assert [(o["to"], o["frm"], o["term"]) for o in out.records] == [(1, 2, 4)]


def random_case(rng, G=6, S=3, n=None, goff=0):
    st = qm.state(num_groups=G, group_offset=goff, num_slots=S,
                  term=[rng.randrange(1, 4) for _ in range(G)],
                  state=[rng.randrange(4) for _ in range(G)],
                  lead=[rng.choice([0, S - 1, qm.NONE, S]) for _ in range(G)],
                  self_slot=[rng.randrange(S) for _ in range(G)])
    recs = []
    for _ in range(rng.randrange(40) if n is None else n):
        t = rng.choice(qm.TYPES + (rng.randrange(256),) * (rng.random() < 0.1))
        recs.append(qm.rec(
            goff + rng.randrange(G + (rng.random() < 0.05)), t,
            rng.choice([rng.randrange(S), qm.NONE, qm.NONE if rng.random() < 0.9 else S]),
            rng.choice([0, 0, rng.randrange(5)]) if t in (qm.TRANSFER_LEADER, qm.READ_INDEX_RESP)
            else (0 if rng.random() < 0.9 else 2),
            rng.randrange(100), rng.getrandbits(64), rng.randrange(3), rng.randrange(1000),
            [(rng.randrange(4), rng.randrange(2), rng.randrange(50))
             for _ in range(rng.choice([0, 0, 1, 3]))]))
    return st, recs


def test_order_free_form_equals_the_sequential_loop():
    rng = random.Random(20240611)
    seen = set()
    for _ in range(1500):
        st, recs = random_case(rng)
        nf, cc = rng.random() < 0.3, rng.choice([0, 2])
        a, b = qm.route(st, recs, nf, cc), qm.route_by_stop(st, recs, nf, cc)
        assert vars(a) == vars(b)
        seen.update(a.disposition)
        # rule 4: one row-writing record per group and pass at most
        closers = [m["group"] for m, d in zip(recs, a.disposition)
                   if d in (qm.ROUTED, qm.STEPDOWN)]
        assert len(closers) == len(set(closers))
    assert seen == set(qm.QD_NAMES)


def test_run_to_end_handles_every_record_once():
    rng = random.Random(7)
    for _ in range(200):
        st, recs = random_case(rng)
        passes = qm.run_to_end(st, recs)
        done = sum(sum(d != qm.DEFERRED for d in p.disposition) for p in passes)
        assert done == len(recs)
        assert not passes or not passes[-1].deferred


def test_vectorised_record_hash_equals_the_scalar_one():
    """record_hashes (what tests/test_gpu_requests.py sums over a list too
    long for the model) against record_hash per record on 1500 random records
    (group ids past 2^33, every disposition, every type and slot byte), and its
    sum over a handled list against route()'s STAT_CHECKSUM."""
    import numpy as np
    rng = np.random.default_rng(4243)
    n = 1500
    group = rng.integers(0, 1 << 62, n, dtype=np.uint64) | np.uint64(1 << 33)
    disp = rng.choice(list(qm.QD_NAMES), n).astype(np.uint8)
    type_ = rng.integers(0, 256, n).astype(np.uint8)
    frm = rng.integers(0, 256, n).astype(np.uint8)
    got = qm.record_hashes(group, disp, type_, frm)
    assert got.dtype == np.uint64 and len(set(got.tolist())) == n
    assert got.tolist() == [qm.record_hash(int(group[i]), int(disp[i]), int(type_[i]),
                                           int(frm[i]), i) for i in range(n)]
    st, recs = random_case(random.Random(11), G=300, n=n, goff=1 << 33)
    o = qm.route(st, recs)
    assert set(o.disposition) == set(qm.QD_NAMES)
    a = lambda k: np.array([m[k] for m in recs], np.uint64)  # noqa: E731
    with np.errstate(over="ignore"):
        total = int(np.add.reduce(qm.record_hashes(a("group"), np.array(o.disposition, np.uint8),
                                                   a("type"), a("from"))))
    assert total == o.stats[qm.STAT_CHECKSUM]
