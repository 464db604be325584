"""The CPU model of qe_follower_step (tests/follower_model.py) against the
reference's own tables (tests/golden/follower_tables.json), the coverage of
the random generator the GPU differential uses, and the entry point's ABI:
exported symbol, struct layouts, argument errors (no GPU needed)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from etcd_amd import _lib
from tests import follower_model as fm
from tests import follower_traces as ft

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "etcd_quorum.h")


def tables():
    with open(os.path.join(HERE, "golden", "follower_tables.json"), encoding="utf-8") as f:
        return json.load(f)


def node_of(log, committed=0, term=0, lead=None, state=fm.ST_FOLLOWER):
    """A node whose storage holds `log` (entries from index 1; the dummy entry
    is (0, 0))."""
    return fm.Node([(0, 0)] + [tuple(e) for e in log], committed=committed, term=term,
                   state=state, lead=fm.NONE_SLOT if lead is None else lead - 1)


def msg_of(m):
    """A fixture message; node id n sits in slot n - 1."""
    ty = {"MsgApp": fm.LMSG_APP, "MsgHeartbeat": fm.LMSG_HEARTBEAT}[m["type"]]
    ents = [tuple(e) for e in m.get("entries", [])]
    assert [i for i, _ in ents] == list(range(m.get("index", 0) + 1, m.get("index", 0) + 1 + len(ents)))
    return fm.Msg(ty, m["from"] - 1, m["term"], m.get("index", 0), m.get("log_term", 0),
                  m["commit"], [(n, t) for n, t in fm_runs([t for _, t in ents])])


def fm_runs(terms):
    runs = []
    for t in terms:
        if runs and runs[-1][1] == t:
            runs[-1][0] += 1
        else:
            runs.append([1, t])
    return runs


def fixture_cases():
    """(id, node, msg) of every fixture row that is a message to a node: the
    rows the GPU test replays too."""
    out = []
    for name, tb in tables().items():
        if tb["level"] not in ("Step", "handleAppendEntries", "handleHeartbeat"):
            continue
        for i, row in enumerate(tb["rows"]):
            log = row.get("follower_log", tb.get("log"))
            out.append((f"{name}#{i}", node_of(log, tb["committed"], tb["term"], tb["lead"]),
                        msg_of(row["msg"])))
    return out


def test_fixture_row_counts():
    t = tables()
    assert {k: len(v["rows"]) for k, v in t.items()} == {
        "TestHandleMsgApp": 11, "TestHandleHeartbeat": 2, "TestLogMaybeAppend": 15,
        "TestFindConflict": 11, "TestFollowerCommitEntry": 4, "TestFollowerCheckMsgApp": 5,
        "TestFollowerAppendEntries": 4, "TestFastLogRejection": 8}
    for v in t.values():
        assert v["source"].startswith("raft/")


def test_handle_msg_app_table():
    tb = tables()["TestHandleMsgApp"]
    for i, row in enumerate(tb["rows"]):
        n, out = fm.step(node_of(tb["log"], tb["committed"], tb["term"]), msg_of(row["msg"]))
        assert n.last_index() == row["want_last_index"], i
        assert n.committed == row["want_committed"], i
        assert (out["result"] == fm.FR_APP_REJECT) == row["want_reject"], i
        assert out["result"] in (fm.FR_APP_REJECT, fm.FR_APP_ACCEPT), i


def test_handle_heartbeat_table():
    tb = tables()["TestHandleHeartbeat"]
    for i, row in enumerate(tb["rows"]):
        n, out = fm.step(node_of(tb["log"], tb["committed"], tb["term"], tb["lead"]),
                         msg_of(row["msg"]))
        assert out["result"] == fm.FR_HEARTBEAT_RESP and out["events"] == fm.TEV_HEARD, i
        assert n.committed == row["want_committed"], i


def test_log_maybe_append_table():
    tb = tables()["TestLogMaybeAppend"]
    panics = 0
    for i, row in enumerate(tb["rows"]):
        n = node_of(tb["log"], tb["log_committed"])
        ents = [tuple(e) for e in row["entries"]]
        if row["want_panic"]:
            with pytest.raises(fm.Refused) as e:
                n.maybe_append(row["index"], row["log_term"], row["committed"], ents, 16)
            assert e.value.code == fm.FR_CONFLICT_COMMITTED, i
            panics += 1
            continue
        lasti, ok, _ = n.maybe_append(row["index"], row["log_term"], row["committed"], ents, 16)
        assert (lasti, ok, n.committed) == (row["want_lasti"], row["want_append"],
                                            row["want_commit"]), i
        if ok and ents:
            assert n.ents[-len(ents):] == ents, i
        n.check()
    assert panics == 1


def test_find_conflict_table():
    tb = tables()["TestFindConflict"]
    for i, row in enumerate(tb["rows"]):
        got = node_of(tb["log"]).find_conflict([tuple(e) for e in row["entries"]])
        assert got == row["want_conflict"], i


def test_follower_commit_entry_table():
    tb = tables()["TestFollowerCommitEntry"]
    for i, row in enumerate(tb["rows"]):
        n, out = fm.step(node_of([], 0, tb["term"], tb["lead"]), msg_of(row["msg"]))
        assert out["result"] == fm.FR_APP_ACCEPT and n.committed == row["want_committed"], i
        assert n.ents[1:] == [tuple(e) for e in row["msg"]["entries"]], i


def test_follower_check_msg_app_table():
    tb = tables()["TestFollowerCheckMsgApp"]
    for i, row in enumerate(tb["rows"]):
        n, out = fm.step(node_of(tb["log"], tb["committed"], tb["term"], tb["lead"]),
                         msg_of(row["msg"]))
        assert out["resp_index"] == row["want_index"], i
        assert (out["result"] == fm.FR_APP_REJECT) == row["want_reject"], i
        # an accepted MsgAppResp carries neither field (zero in the reference)
        assert out.get("reject_hint", 0) == row["want_reject_hint"], i
        assert out.get("resp_log_term", 0) == row["want_log_term"], i


def test_follower_append_entries_table():
    tb = tables()["TestFollowerAppendEntries"]
    for i, row in enumerate(tb["rows"]):
        n, out = fm.step(node_of(tb["log"], tb["committed"], tb["term"], tb["lead"]),
                         msg_of(row["msg"]))
        assert out["result"] == fm.FR_APP_ACCEPT, i
        assert n.ents[1:] == [tuple(e) for e in row["want_entries"]], i


def test_fast_log_rejection_follower_half():
    tb = tables()["TestFastLogRejection"]
    for i, row in enumerate(tb["rows"]):
        n0 = node_of(row["follower_log"], tb["committed"], tb["term"], tb["lead"])
        n, out = fm.step(n0, msg_of(row["msg"]))
        assert out["result"] == fm.FR_APP_REJECT and out["events"] == fm.TEV_RESET, i
        assert (n.term, n.lead, n.ents) == (1, 0, n0.ents), i
        assert out["reject_hint"] == row["want_reject_hint"], i
        assert out["resp_log_term"] == row["want_log_term"], i


def test_conflict_committed_needs_a_call_below_the_handler():
    """handleAppendEntries answers index < committed before maybeAppend runs,
    and every entry of a message lies above its index: through a message the
    panic row of TestLogMaybeAppend is QE_FR_APP_STALE, and
    QE_FR_CONFLICT_COMMITTED is a guard no well-formed state reaches."""
    tb = tables()["TestLogMaybeAppend"]
    row = [r for r in tb["rows"] if r["want_panic"]][0]
    m = fm.Msg(fm.LMSG_APP, 1, 3, row["index"], row["log_term"], row["committed"], [(1, 4)])
    n, out = fm.step(node_of(tb["log"], tb["log_committed"], 3), m)
    assert out["result"] == fm.FR_APP_STALE and out["resp_index"] == tb["log_committed"]


def test_interaction_traces_from_the_receivers_side():
    """tests/follower_traces.py compares every response, HardState and entry
    list while it replays; here the coverage: all 71 received MsgApps (12 of
    them rejected) and all 4 MsgHeartbeats of the fixture, nothing skipped
    beyond the explicit table."""
    steps, skipped = ft.replay_all()
    assert len(ft.SKIP) <= ft.MAX_SKIP and len(skipped) == len(ft.SKIP)
    apps = [s for s in steps if s.msg.type == fm.LMSG_APP]
    beats = [s for s in steps if s.msg.type == fm.LMSG_HEARTBEAT]
    assert len(apps) + len(beats) + len(skipped) == 71 + 4
    assert sum(s.out["result"] == fm.FR_APP_REJECT for s in apps) == 12
    assert len(beats) == 4 and all(s.out["result"] == fm.FR_HEARTBEAT_RESP for s in beats)
    # the traces reach a truncation (probe_and_replicate.txt) and a fresh node's first append
    assert any(s.out.get("append_from") and s.out["append_from"] <= s.before.last_index()
               for s in apps)
    assert any(s.before.last_index() == 0 for s in apps)


@pytest.mark.parametrize("R,E", [(1, 0), (1, 4), (4, 1), (4, 4), (16, 4)])
def test_generator_steps_cleanly(R, E):
    rng = np.random.default_rng(R * 16 + E)
    nodes = [fm.gen_node(rng, R, 5) for _ in range(300)]
    for _ in range(4):
        msgs = [fm.gen_msg(rng, n, E, 5) for n in nodes]
        nodes, outs, _ = fm.step_batch(nodes, msgs, 0, 5, R)
        for n in nodes:
            n.check()
            assert len(n.runs) <= R and n.ents[0][0] <= n.committed <= n.last_index()


def test_generator_coverage():
    """Every QE_FR_* code the entry point can return, a truncation that drops
    two or more runs, an append that creates two or more."""
    seen, dropped2, created2 = set(), False, False
    for R, E, flags in ((1, 4, 0), (4, 1, 1), (4, 4, 2), (16, 4, 3), (16, 0, 0)):
        rng = np.random.default_rng(1000 + R + E)
        nodes = [fm.gen_node(rng, R, 5) for _ in range(1500)]
        for _ in range(4):
            msgs = [fm.gen_msg(rng, n, E, 5) for n in nodes]
            after, outs, _ = fm.step_batch(nodes, msgs, flags, 5, R)
            for a, b, o in zip(nodes, after, outs):
                seen.add(o["result"])
                ci = o.get("append_from", 0)
                if ci:
                    kept = len([r for r in a.runs if r[0] < ci])
                    dropped2 |= len(a.runs) - kept >= 2
                    created2 |= len(b.runs) - kept >= 2
            nodes = after
    want = set(fm.FR_NAMES) - {fm.FR_CONFLICT_COMMITTED}  # (unreachable, see above)
    assert seen == want, sorted(fm.FR_NAMES[c] for c in want - seen)
    assert dropped2 and created2


# ---------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------
def test_symbol_exported():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert " qe_follower_step" in out


LAYOUT_PROG = r"""
#include <stdio.h>
#include <stddef.h>
#include "etcd_quorum.h"
#define F(T, m) printf(#T " " #m " %zu\n", offsetof(T, m));
#define Z(T) printf(#T " sizeof %zu\n", sizeof(T));
int main(void) {
  Z(qe_follower) F(qe_follower, term) F(qe_follower, state) F(qe_follower, lead)
  F(qe_follower, vote) F(qe_follower, flags)
  Z(qe_leader_msgs) F(qe_leader_msgs, type) F(qe_leader_msgs, term) F(qe_leader_msgs, index)
  F(qe_leader_msgs, log_term) F(qe_leader_msgs, commit) F(qe_leader_msgs, msg_runs)
  F(qe_leader_msgs, ent_len) F(qe_leader_msgs, ent_term)
  Z(qe_follower_out) F(qe_follower_out, result) F(qe_follower_out, resp_index)
  F(qe_follower_out, reject_hint) F(qe_follower_out, resp_log_term)
  F(qe_follower_out, append_from) F(qe_follower_out, events)
  printf("qe_leader_msgs from_ %zu\n", offsetof(qe_leader_msgs, from));
  printf("const QE_MAX_MSG_RUNS %d\nconst QE_FR_REFUSED %d\nconst QE_FR_BAD_MSG %d\n",
         QE_MAX_MSG_RUNS, QE_FR_REFUSED, QE_FR_BAD_MSG);
  printf("const QE_FR_COMMIT_PAST_LOG %d\nconst QE_FR_CONFLICT_COMMITTED %d\n",
         QE_FR_COMMIT_PAST_LOG, QE_FR_CONFLICT_COMMITTED);
  printf("const QE_FR_RUNS_FULL %d\nconst QE_FR_APP_GAP %d\nconst QE_FR_APP_STALE %d\n",
         QE_FR_RUNS_FULL, QE_FR_APP_GAP, QE_FR_APP_STALE);
  printf("const QE_FR_APP_ACCEPT %d\nconst QE_FR_APP_REJECT %d\nconst QE_FR_HEARTBEAT_RESP %d\n",
         QE_FR_APP_ACCEPT, QE_FR_APP_REJECT, QE_FR_HEARTBEAT_RESP);
  printf("const QE_FR_LOWER_TERM_RESP %d\nconst QE_FR_IGNORED %d\nconst QE_LMSG_APP %d\n",
         QE_FR_LOWER_TERM_RESP, QE_FR_IGNORED, QE_LMSG_APP);
  printf("const QE_LMSG_HEARTBEAT %d\nconst QE_STAT_FOLLOW_APPENDED %d\n", QE_LMSG_HEARTBEAT,
         (int)QE_STAT_FOLLOW_APPENDED);
  return 0;
}
"""


def test_struct_layout_and_constants_match_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_PROG)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)])
    ctypes_of = {"qe_follower": _lib.QeFollower, "qe_leader_msgs": _lib.QeLeaderMsgs,
                 "qe_follower_out": _lib.QeFollowerOut}
    n = 0
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        t, m, v = line.split()
        n += 1
        if t == "const":
            assert getattr(_lib, m) == int(v), m
            assert getattr(fm, m[3:], int(v)) == int(v), m  # the model's own copy
        elif m == "sizeof":
            assert C.sizeof(ctypes_of[t]) == int(v), t
        else:
            assert getattr(ctypes_of[t], m).offset == int(v), (t, m)
    assert n == 39


class _Args:
    """A complete, valid argument set over host memory no kernel ever sees:
    every case below must be turned away before a launch."""

    def __init__(self, G=4):
        self.keep = []
        u64 = lambda n=G: self.buf(C.c_uint64, n)  # noqa: E731
        u8 = lambda n=G: self.buf(C.c_uint8, n)  # noqa: E731
        self.p = _lib.QeProgress(num_groups=G, num_slots=3, inflight_cap=1, stride=G,
                                 committed=u64(), last_index=u64(), log_runs=2,
                                 run_first=u64(2 * G), run_term=u64(2 * G), run_count=u8())
        self.f = _lib.QeFollower(term=u64(), state=u8(), lead=u8(), vote=u8(), flags=0)
        self.m = _lib.QeLeaderMsgs(type=u8(), from_=u8(), term=u64(), index=u64(), log_term=u64(),
                                   commit=u64(), msg_runs=1, ent_len=self.buf(C.c_uint32, G),
                                   ent_term=u64())
        self.o = _lib.QeFollowerOut(result=u8())

    def buf(self, ty, n):
        b = (ty * n)()
        self.keep.append(b)
        return C.cast(b, C.c_void_p)

    def call(self, p=True, f=True, m=True, o=True):
        r = lambda x, on: C.byref(x) if on else None  # noqa: E731
        return _lib.lib().qe_follower_step(r(self.p, p), r(self.f, f), r(self.m, m),
                                           r(self.o, o), None, None)


def test_argument_errors_without_gpu():
    for which in ("p", "f", "m", "o"):
        assert _Args().call(**{which: False}) == _lib.QE_EINVAL, which
    rows = [("p", k) for k in ("committed", "last_index", "run_first", "run_term", "run_count")]
    rows += [("f", k) for k in ("term", "state", "lead")]
    rows += [("m", k) for k in ("type", "from_", "term", "index", "log_term", "commit",
                                "ent_len", "ent_term")]
    rows += [("o", "result")]
    for st, field in rows:
        a = _Args()
        setattr(getattr(a, st), field, None)
        assert a.call() == _lib.QE_EINVAL, (st, field)
    for st, field, val in (("m", "msg_runs", _lib.QE_MAX_MSG_RUNS + 1), ("p", "log_runs", 0),
                           ("p", "log_runs", _lib.QE_MAX_LOG_RUNS + 1), ("p", "stride", 3),
                           ("f", "flags", 4), ("f", "flags", 0x80000001), ("p", "num_slots", 0),
                           ("p", "num_slots", 17)):
        a = _Args()
        setattr(getattr(a, st), field, val)
        assert a.call() == _lib.QE_EINVAL, (st, field, val)
    # nothing to do is not an error; the optional rows may be absent
    a = _Args()
    a.p.num_groups = 0
    assert a.call() == _lib.QE_OK
    a = _Args()
    a.p.num_groups, a.f.vote, a.m.msg_runs, a.m.ent_len, a.m.ent_term = 0, None, 0, None, None
    assert a.call() == _lib.QE_OK
