"""The C surface of qe_inbox: symbols, struct layout against the ctypes mirror,
every constant, the scratch-size formula and every QE_EINVAL / QE_ERANGE the
header lists.  Validation happens before any HIP call, so the argument errors
need no GPU (the pointers are never read)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from etcd_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "etcd_quorum.h")
V = C.c_void_p(64)  # any non-NULL pointer

IN_FIELDS = [f for f, _ in _lib.QeInboxIn._fields_]
OUT_FIELDS = [f for f, _ in _lib.QeInboxOut._fields_]
CONSTANTS = ["QE_IMSG_APP", "QE_IMSG_SNAP", "QE_IMSG_HEARTBEAT", "QE_IMSG_APP_RESP",
             "QE_IMSG_APP_RESP_REJECT", "QE_IMSG_HEARTBEAT_RESP", "QE_IMSG_SNAP_STATUS",
             "QE_IMSG_SNAP_STATUS_REJECT", "QE_IMSG_UNREACHABLE", "QE_IMSG_TRANSFER_LEADER",
             "QE_IMSG_VOTE", "QE_IMSG_PREVOTE", "QE_IMSG_VOTE_RESP", "QE_IMSG_PREVOTE_RESP",
             "QE_IMSG_TIMEOUT_NOW", "QE_IMSG_HUP", "QE_ID_ROUTED", "QE_ID_STEPDOWN",
             "QE_ID_DEFERRED", "QE_ID_DROP_LOWER_TERM", "QE_ID_DROP_NOT_LEADER", "QE_ID_BAD",
             "QE_INBOX_SRC_TICK", "QE_STAT_INBOX_ROUTED", "QE_STAT_INBOX_STEPDOWN",
             "QE_STAT_INBOX_DEFERRED", "QE_STAT_INBOX_LOWER_TERM", "QE_STAT_INBOX_NOT_LEADER",
             "QE_STAT_INBOX_BAD"]
LAYOUT_PROG = r"""
#include <stdio.h>
#include <stddef.h>
#include "etcd_quorum.h"
#define F(T, m) printf(#T " " #m " %zu\n", offsetof(T, m));
#define Z(T) printf(#T " sizeof %zu\n", sizeof(T));
#define K(c) printf(#c " value %llu\n", (unsigned long long)(c));
int main(void) {
  Z(qe_inbox_in) Z(qe_inbox_out)
""" + "\n".join(f"  F(qe_inbox_in, {'from' if f == 'from_' else f})" for f in IN_FIELDS) + "\n" + \
    "\n".join(f"  F(qe_inbox_out, {f})" for f in OUT_FIELDS) + "\n" + \
    "\n".join(f"  K({c})" for c in CONSTANTS) + "\n  return 0;\n}\n"
CTYPES = {"qe_inbox_in": _lib.QeInboxIn, "qe_inbox_out": _lib.QeInboxOut}


def test_symbols_and_prototypes():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = set(re.findall(r"\s[TW]\s+(qe_\w+)", out))
    assert {"qe_inbox", "qe_inbox_scratch_bytes"} <= exported
    assert {"qe_inbox", "qe_inbox_scratch_bytes"} <= set(_lib.PROTOTYPES)
    assert _lib.lib().qe_abi_version() == 8  # additive: the version stays


def test_scratch_size_formula():
    """4 * (3 + S) * G bytes of words, n flag bytes and qe_collect's part for n
    flags; 0 for a slot count no call accepts."""
    L = _lib.lib()
    for G in (0, 1, 4097, 1 << 24):
        for S in (1, 5, 16):
            for n in (0, 1, 4096, 4097, 0xFFFFFFF0):
                assert L.qe_inbox_scratch_bytes(G, S, n) == \
                    4 * (3 + S) * G + n + L.qe_collect_scratch_bytes(n), (G, S, n)
    assert L.qe_inbox_scratch_bytes(100, 0, 10) == 0 == L.qe_inbox_scratch_bytes(100, 17, 10)
    assert L.qe_inbox_scratch_bytes(1 << 24, 5, 0) - L.qe_collect_scratch_bytes(0) == 512 << 20


def test_struct_layout_and_constants_match_header(tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_PROG)
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.dirname(HEADER), str(src), "-o",
                           str(exe)])
    seen = {}
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        t, m, v = line.split()
        if m == "value":
            seen[t] = int(v)
        elif m == "sizeof":
            assert C.sizeof(CTYPES[t]) == int(v), t
        else:
            assert getattr(CTYPES[t], "from_" if m == "from" else m).offset == int(v), (t, m)
    assert seen == {c: getattr(_lib, c) for c in CONSTANTS}
    # the values the issue fixes: the list types, the classes' ranges, the dispositions
    assert [seen[c] for c in CONSTANTS[:16]] == list(range(1, 17))
    assert [seen[c] for c in CONSTANTS[16:22]] == [1, 2, 3, 4, 5, 255]
    assert (seen["QE_IMSG_APP"], seen["QE_IMSG_SNAP"], seen["QE_IMSG_HEARTBEAT"]) == \
        (_lib.QE_OMSG_APP, _lib.QE_OMSG_SNAP, _lib.QE_OMSG_HEARTBEAT)
    assert seen["QE_INBOX_SRC_TICK"] == 0xFFFFFFFF
    stats = [seen[c] for c in CONSTANTS if c.startswith("QE_STAT_INBOX")]
    assert len(set(stats) | {0, 14, 15}) == len(stats) + 3  # no counter is shared


OPTIONAL_OUT = ("v_flags", "r_ctx", "f_src", "s_src", "v_src", "r_src")


def good():
    """A call every check passes (G = 4, S = 3, n = 8, E = 2)."""
    p = dict(num_groups=4, num_slots=3, stride=4)
    f = dict(term=V, state=V)
    i = dict(num_records=8, msg_runs=2, group=V, from_=V, type=V, term=V, index=V, log_term=V,
             commit=V, hint=V, ctx=None, flags=None, ent_len=V, ent_term=V, tick_action=None)
    o = {k: (None if k in OPTIONAL_OUT else V) for k in OUT_FIELDS}
    return p, f, i, o


def call(p, f, i, o, scratch=V, null=()):
    L = _lib.lib()
    ps, fs = _lib.QeProgress(**p), _lib.QeFollower(**f)
    ins, outs = _lib.QeInboxIn(**i), _lib.QeInboxOut(**o)
    arg = lambda name, s: None if name in null else C.byref(s)  # noqa: E731
    return L.qe_inbox(arg("p", ps), arg("f", fs), arg("in", ins), arg("out", outs), scratch, None,
                      None)


BAD = {
    "NULL p": lambda p, f, i, o: dict(null=("p",)),
    "NULL f": lambda p, f, i, o: dict(null=("f",)),
    "NULL in": lambda p, f, i, o: dict(null=("in",)),
    "NULL out": lambda p, f, i, o: dict(null=("out",)),
    "NULL scratch": lambda p, f, i, o: dict(scratch=None),
    "scratch not 8-B aligned": lambda p, f, i, o: dict(scratch=C.c_void_p(68)),
    "NULL f.term": lambda p, f, i, o: f.update(term=None),
    "NULL f.state": lambda p, f, i, o: f.update(state=None),
    "msg_runs > QE_MAX_MSG_RUNS": lambda p, f, i, o: i.update(msg_runs=5),
    "msg_runs without in.ent_len": lambda p, f, i, o: i.update(ent_len=None),
    "msg_runs without in.ent_term": lambda p, f, i, o: i.update(ent_term=None),
    "msg_runs without out.f_ent_len": lambda p, f, i, o: o.update(f_ent_len=None),
    "msg_runs without out.f_ent_term": lambda p, f, i, o: o.update(f_ent_term=None),
    "stride < num_groups": lambda p, f, i, o: p.update(stride=3),
    "num_slots 0": lambda p, f, i, o: p.update(num_slots=0),
    "num_slots 17": lambda p, f, i, o: p.update(num_slots=17),
    "in.reserved": lambda p, f, i, o: i.update(reserved=1),
    "p.reserved": lambda p, f, i, o: p.update(reserved=1),
    "p.reserved2": lambda p, f, i, o: p.update(reserved2=1),
}
for _k in ("group", "from_", "type", "term", "index", "log_term", "commit", "hint"):
    BAD[f"num_records > 0 with NULL in.{_k}"] = lambda p, f, i, o, k=_k: i.update(**{k: None})
for _k in OUT_FIELDS:
    if _k not in OPTIONAL_OUT + ("f_ent_len", "f_ent_term"):
        BAD[f"NULL out.{_k}"] = lambda p, f, i, o, k=_k: o.update(**{k: None})


@pytest.mark.parametrize("case", sorted(BAD))
def test_einval(case):
    p, f, i, o = good()
    kw = BAD[case](p, f, i, o)
    assert call(p, f, i, o, **(kw if isinstance(kw, dict) else {})) == _lib.QE_EINVAL, case


def test_erange():
    """Positions are 32-bit keys: num_records above 0xFFFFFFF0."""
    p, f, i, o = good()
    i.update(num_records=0xFFFFFFF1)
    assert call(p, f, i, o) == _lib.QE_ERANGE
    i.update(num_records=1 << 40)
    assert call(p, f, i, o) == _lib.QE_ERANGE


def test_einval_holds_for_an_empty_batch_and_an_empty_list():
    """num_groups == 0 skips no check but scratch's; num_records == 0 none but
    the record arrays'."""
    for field in ("disposition", "deferred", "deferred_count", "v_type", "r_type"):
        p, f, i, o = good()
        p.update(num_groups=0, stride=0)
        o.update(**{field: None})
        assert call(p, f, i, o, scratch=None) == _lib.QE_EINVAL, field
        p, f, i, o = good()
        i.update(num_records=0, group=None, from_=None, type=None, term=None, index=None,
                 log_term=None, commit=None, hint=None)
        o.update(**{field: None})
        assert call(p, f, i, o) == _lib.QE_EINVAL, field
    p, f, i, o = good()
    p.update(num_groups=0, stride=0)
    assert call(p, f, i, o, scratch=C.c_void_p(12)) == _lib.QE_EINVAL


def test_empty_batch():
    """num_groups == 0 is QE_OK with *deferred_count = 0.  The zero is a device
    write: with a device it is checked; without one the call still passes
    every argument check (it fails in the runtime, not with QE_EINVAL)."""
    import torch

    p, f, i, o = good()
    p.update(num_groups=0, stride=0)
    if torch.cuda.is_available():
        count = torch.full((1,), 77, dtype=torch.int64, device="cuda")
        o.update(deferred_count=C.c_void_p(count.data_ptr()))
        assert call(p, f, i, o, scratch=None) == _lib.QE_OK
        torch.cuda.synchronize()
        assert int(count.item()) == 0
    else:
        host = C.c_uint64(77)
        o.update(deferred_count=C.cast(C.pointer(host), C.c_void_p))
        assert call(p, f, i, o, scratch=None) in (_lib.QE_OK, _lib.QE_EHIP)
