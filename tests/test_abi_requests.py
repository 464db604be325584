"""The C surface of qe_requests: symbols, struct layout against the ctypes
mirror, every constant, the scratch-size formula and every QE_EINVAL /
QE_ERANGE the header lists.  Validation happens before any HIP call, so the
argument errors need no GPU (the pointers are never read)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from etcd_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "etcd_quorum.h")
V = C.c_void_p(64)  # any non-NULL pointer

IN_FIELDS = [f for f, _ in _lib.QeRequestsIn._fields_]
OUT_FIELDS = [f for f, _ in _lib.QeRequestsOut._fields_]
TYPES = ["QE_QMSG_TRANSFER_LEADER", "QE_QMSG_PROP", "QE_QMSG_READ_INDEX", "QE_QMSG_READ_INDEX_RESP"]
DISPOSITIONS = ["QE_QD_ROUTED", "QE_QD_STEPDOWN", "QE_QD_DEFERRED", "QE_QD_DROP_LOWER_TERM",
                "QE_QD_NO_ARM", "QE_QD_FORWARDED", "QE_QD_READ_STATE", "QE_QD_PROP_DROPPED",
                "QE_QD_NO_LEADER", "QE_QD_REF_PANIC", "QE_QD_BAD"]
KINDS = ["QE_QO_FWD", "QE_QO_READ_STATE", "QE_QO_PROP_DROPPED"]
STATS = ["QE_STAT_REQ_BAD", "QE_STAT_REQ_NO_ARM", "QE_STAT_REQ_NO_LEADER", "QE_STAT_REQ_ROUTED",
         "QE_STAT_REQ_LOWER_TERM", "QE_STAT_REQ_DEFERRED", "QE_STAT_REQ_FORWARDED",
         "QE_STAT_REQ_PROP_DROPPED", "QE_STAT_REQ_READ_STATE", "QE_STAT_REQ_REF_PANIC",
         "QE_STAT_REQ_STEPDOWN"]
CONSTANTS = TYPES + DISPOSITIONS + KINDS + STATS + ["QE_REQ_NO_FORWARD"]
cname = lambda f: "from" if f == "from_" else f  # noqa: E731
LAYOUT_PROG = r"""
#include <stdio.h>
#include <stddef.h>
#include "etcd_quorum.h"
#define F(T, m) printf(#T " " #m " %zu\n", offsetof(T, m));
#define Z(T) printf(#T " sizeof %zu\n", sizeof(T));
#define K(c) printf(#c " value %llu\n", (unsigned long long)(c));
int main(void) {
  Z(qe_requests_in) Z(qe_requests_out)
""" + "\n".join(f"  F(qe_requests_in, {cname(f)})" for f in IN_FIELDS) + "\n" + \
    "\n".join(f"  F(qe_requests_out, {cname(f)})" for f in OUT_FIELDS) + "\n" + \
    "\n".join(f"  K({c})" for c in CONSTANTS + ["QE_IMSG_TRANSFER_LEADER", "QE_IMSG_HUP"]) + \
    "\n  return 0;\n}\n"
CTYPES = {"qe_requests_in": _lib.QeRequestsIn, "qe_requests_out": _lib.QeRequestsOut}


def test_symbols_and_prototypes():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = set(re.findall(r"\s[TW]\s+(qe_\w+)", out))
    assert {"qe_requests", "qe_requests_scratch_bytes"} <= exported
    assert {"qe_requests", "qe_requests_scratch_bytes"} <= set(_lib.PROTOTYPES)
    assert _lib.lib().qe_abi_version() == 8  # additive: the version stays


def test_scratch_size_formula():
    """One 4-B word per group (qe_inbox: 3 + S of them), two flag bytes per
    record and qe_collect's part for n flags once per list; no term in S."""
    L = _lib.lib()
    for G in (0, 1, 4097, 1 << 24):
        for n in (0, 1, 4096, 4097, 0xFFFFFFF0):
            assert L.qe_requests_scratch_bytes(G, n) == \
                4 * G + 2 * n + 2 * L.qe_collect_scratch_bytes(n), (G, n)
    words = L.qe_requests_scratch_bytes(1 << 24, 0) - 2 * L.qe_collect_scratch_bytes(0)
    assert words == 64 << 20 <= 4 * (1 << 24)
    assert (L.qe_inbox_scratch_bytes(1 << 24, 5, 0) - L.qe_collect_scratch_bytes(0)) == 8 * words


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
    assert {c: seen[c] for c in CONSTANTS} == {c: getattr(_lib, c) for c in CONSTANTS}
    # the values the issue fixes: the types continue the QE_IMSG_* numbering
    assert [seen[c] for c in TYPES] == [10, 17, 18, 19]
    assert seen["QE_QMSG_TRANSFER_LEADER"] == seen["QE_IMSG_TRANSFER_LEADER"]
    assert seen["QE_QMSG_PROP"] == seen["QE_IMSG_HUP"] + 1
    assert [seen[c] for c in DISPOSITIONS] == list(range(1, 11)) + [255]
    assert [seen[c] for c in DISPOSITIONS[:4]] == \
        [_lib.QE_ID_ROUTED, _lib.QE_ID_STEPDOWN, _lib.QE_ID_DEFERRED, _lib.QE_ID_DROP_LOWER_TERM]
    assert [seen[c] for c in KINDS] == [1, 2, 3]
    assert seen["QE_REQ_NO_FORWARD"] == 1
    stats = [seen[c] for c in STATS]
    assert len(set(stats) | {0, 14, 15}) == len(stats) + 3  # no counter is shared
    # the names qe_inbox has too alias the same counters
    for c in ("ROUTED", "STEPDOWN", "DEFERRED", "LOWER_TERM", "BAD"):
        assert seen["QE_STAT_REQ_" + c] == getattr(_lib, "QE_STAT_INBOX_" + c)


OPTIONAL_OUT = ("p_payload", "p_cc_count", "p_cc_pos", "p_cc_leave", "p_cc_size", "v_flags",
                "p_src", "ri_src", "v_src", "r_src")
LIST_OUT = ("group", "kind", "type", "to", "from_", "term", "index", "key", "src")


def good():
    """A call every check passes (G = 4, S = 3, n = 8, max_cc = 2, capacity 8)."""
    p = dict(num_groups=4, num_slots=3, stride=4, self_slot=V)
    f = dict(term=V, state=V, lead=V)
    i = dict(num_records=8, max_cc=2, flags=_lib.QE_REQ_NO_FORWARD, group=V, type=V, from_=V,
             term=V, index=V, key=V, num_entries=V, payload=None, cc_count=V, cc_pos=V, cc_leave=V,
             cc_size=V, reserved=0)
    o = {k: V for k in OUT_FIELDS}
    o.update(cc_stride=4, capacity=8, p_payload=None, v_flags=None, p_src=None, ri_src=None,
             v_src=None, r_src=None)
    return p, f, i, o


def call(p, f, i, o, scratch=V, null=()):
    L = _lib.lib()
    ps, fs = _lib.QeProgress(**p), _lib.QeFollower(**f)
    ins, outs = _lib.QeRequestsIn(**i), _lib.QeRequestsOut(**o)
    arg = lambda name, s: None if name in null else C.byref(s)  # noqa: E731
    return L.qe_requests(arg("p", ps), arg("f", fs), arg("in", ins), arg("out", outs), scratch,
                         None, None)


BAD = {
    "NULL p": lambda p, f, i, o: dict(null=("p",)),
    "NULL f": lambda p, f, i, o: dict(null=("f",)),
    "NULL in": lambda p, f, i, o: dict(null=("in",)),
    "NULL out": lambda p, f, i, o: dict(null=("out",)),
    "NULL scratch": lambda p, f, i, o: dict(scratch=None),
    "scratch not 8-B aligned": lambda p, f, i, o: dict(scratch=C.c_void_p(68)),
    "NULL f.term": lambda p, f, i, o: f.update(term=None),
    "NULL f.state": lambda p, f, i, o: f.update(state=None),
    "NULL f.lead": lambda p, f, i, o: f.update(lead=None),
    "NULL p.self_slot": lambda p, f, i, o: p.update(self_slot=None),
    "max_cc > QE_PROP_MAX_CC": lambda p, f, i, o: i.update(max_cc=_lib.QE_PROP_MAX_CC + 1),
    "cc_stride < num_groups": lambda p, f, i, o: o.update(cc_stride=3),
    "stride < num_groups": lambda p, f, i, o: p.update(stride=3),
    "num_slots 0": lambda p, f, i, o: p.update(num_slots=0),
    "num_slots 17": lambda p, f, i, o: p.update(num_slots=17),
    "in.reserved": lambda p, f, i, o: i.update(reserved=1),
    "in.reserved high half": lambda p, f, i, o: i.update(reserved=1 << 32),
    "in.flags unknown bit": lambda p, f, i, o: i.update(flags=2),
    "p.reserved": lambda p, f, i, o: p.update(reserved=1),
    "p.reserved2": lambda p, f, i, o: p.update(reserved2=1),
}
for _k in ("group", "type", "from_", "term", "index", "key"):
    BAD[f"num_records > 0 with NULL in.{_k}"] = lambda p, f, i, o, k=_k: i.update(**{k: None})
for _k in ("cc_pos", "cc_leave", "cc_size"):
    BAD[f"max_cc and cc_count with NULL in.{_k}"] = lambda p, f, i, o, k=_k: i.update(**{k: None})
    BAD[f"max_cc with NULL out.p_{_k}"] = lambda p, f, i, o, k=_k: o.update(**{"p_" + k: None})
BAD["max_cc with NULL out.p_cc_count"] = lambda p, f, i, o: o.update(p_cc_count=None)
for _k in OUT_FIELDS:
    if _k not in OPTIONAL_OUT + LIST_OUT + ("cc_stride", "capacity"):
        BAD[f"NULL out.{_k}"] = lambda p, f, i, o, k=_k: o.update(**{k: None})
for _k in LIST_OUT:
    BAD[f"capacity > 0 with NULL out.{_k}"] = lambda p, f, i, o, k=_k: o.update(**{k: None})


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
    for field in ("disposition", "deferred", "deferred_count", "count", "v_type", "r_type",
                  "p_num_entries", "ri_request"):
        p, f, i, o = good()
        p.update(num_groups=0, stride=0)
        o.update(**{field: None})
        assert call(p, f, i, o, scratch=None) == _lib.QE_EINVAL, field
        p, f, i, o = good()
        i.update(num_records=0, group=None, type=None, from_=None, term=None, index=None, key=None)
        o.update(**{field: None})
        assert call(p, f, i, o) == _lib.QE_EINVAL, field
    p, f, i, o = good()
    p.update(num_groups=0, stride=0)
    assert call(p, f, i, o, scratch=C.c_void_p(12)) == _lib.QE_EINVAL


def test_what_may_be_null_is_accepted_up_to_the_first_hip_call():
    """The optional pointers pass every check: with an empty batch the call
    reaches the runtime (QE_OK with a device, QE_EHIP without)."""
    import torch

    p, f, i, o = good()
    p.update(num_groups=0, stride=0)
    i.update(max_cc=0, num_entries=None, payload=None, cc_count=None, cc_pos=None, cc_leave=None,
             cc_size=None, flags=0)
    o.update(capacity=0, cc_stride=0, **{k: None for k in OPTIONAL_OUT + LIST_OUT})
    if torch.cuda.is_available():
        counts = torch.full((2,), 77, dtype=torch.int64, device="cuda")
        o.update(deferred_count=C.c_void_p(counts.data_ptr()),
                 count=C.c_void_p(counts.data_ptr() + 8))
        assert call(p, f, i, o, scratch=None) == _lib.QE_OK
        torch.cuda.synchronize()
        assert counts.tolist() == [0, 0]
    else:
        host = (C.c_uint64 * 2)(77, 77)
        o.update(deferred_count=C.cast(host, C.c_void_p),
                 count=C.c_void_p(C.addressof(host) + 8))
        assert call(p, f, i, o, scratch=None) in (_lib.QE_OK, _lib.QE_EHIP)
