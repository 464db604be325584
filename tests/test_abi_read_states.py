"""The C surface of qe_read_note / qe_read_states: symbols, struct layout against
the ctypes mirror, the constants with their statistics aliases, and every
QE_EINVAL / QE_ERANGE the header lists.  Validation happens before any HIP call, so the
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
BOOK_FIELDS = ("req_index", "req_from")
IN_ROWS = ("read_released", "term_commit", "term_commit_index", "ri_result", "ri_index", "ri_from",
           "ri_key")
IN_FIELDS = IN_ROWS + ("reserved",)
RECORD_FIELDS = ("group", "kind", "to", "ctx", "index")
OUT_FIELDS = ("capacity",) + RECORD_FIELDS + ("key", "count")
STRUCTS = {"qe_read_book": (BOOK_FIELDS, _lib.QeReadBook),
           "qe_read_states_in": (IN_FIELDS, _lib.QeReadStatesIn),
           "qe_read_states_out": (OUT_FIELDS, _lib.QeReadStatesOut)}

LAYOUT_PROG = r"""
#include <stdio.h>
#include <stddef.h>
#include "etcd_quorum.h"
#define F(T, m) printf(#T " " #m " %zu\n", offsetof(T, m));
#define Z(T) printf(#T " sizeof %zu\n", sizeof(T));
int main(void) {
""" + "\n".join(f"  Z({t}) " + " ".join(f"F({t}, {k})" for k in fs)
                for t, (fs, _) in STRUCTS.items()) + r"""
  printf("QE_RS %d %d\n", QE_RS_STATE | QE_RS_RESP << 8, QE_RS_TERM_COMMIT);
  printf("QE_STAT_READ %d %d\n", QE_STAT_READ_STATE | QE_STAT_READ_RESP << 8,
         QE_STAT_READ_TERM_COMMIT);
  printf("QE_STAT_SAME %d %d\n", QE_STAT_READ_STATE == QE_STAT_VOTE_WON &&
         QE_STAT_READ_RESP == QE_STAT_VOTE_PENDING,
         QE_STAT_READ_TERM_COMMIT == QE_STAT_COMMIT_ADVANCED);
  printf("QE_READ %d %d\n", QE_READ_QUEUE, QE_READ_CAP_MAX);
  return 0;
}
"""
NAMES = {"qe_read_note", "qe_read_states", "qe_read_states_scratch_bytes"}


def test_symbols_and_prototypes():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = set(re.findall(r"\s[TW]\s+(qe_\w+)", out))
    assert NAMES <= exported and NAMES <= set(_lib.PROTOTYPES)
    with open(HEADER, encoding="utf-8") as f:
        text = f.read()
    for n in NAMES:
        assert re.search(rf"^(int|size_t) {n}\(", text, re.M), n
    L = _lib.lib()
    assert L.qe_abi_version() == 8  # additive: the version stays
    for G in (0, 1, 4096, 4097, 1 << 24):  # qe_collect's part alone
        assert L.qe_read_states_scratch_bytes(G) == L.qe_collect_scratch_bytes(G)


def test_struct_layout_and_constants_match_header(tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_PROG)
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.dirname(HEADER), str(src), "-o",
                           str(exe)])
    seen, fields = {}, {t: [] for t in STRUCTS}
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        t, m, v = line.split()
        if t.startswith("QE_"):
            seen[t] = (int(m), int(v))
        elif m == "sizeof":
            assert C.sizeof(STRUCTS[t][1]) == int(v), t
        else:
            assert getattr(STRUCTS[t][1], m).offset == int(v), (t, m)
            fields[t].append(m)
    for t, (fs, ct) in STRUCTS.items():
        assert fields[t] == list(fs) == [k for k, _ in ct._fields_], t
    L = _lib
    assert seen["QE_RS"] == (L.QE_RS_STATE | L.QE_RS_RESP << 8, L.QE_RS_TERM_COMMIT)
    assert seen["QE_STAT_READ"] == (L.QE_STAT_READ_STATE | L.QE_STAT_READ_RESP << 8,
                                    L.QE_STAT_READ_TERM_COMMIT)
    assert seen["QE_STAT_SAME"] == (1, 1)
    assert seen["QE_READ"] == (L.QE_READ_QUEUE, L.QE_READ_CAP_MAX)
    # the aliases name the counters the other lists use for their kinds
    assert L.QE_STAT_READ_STATE == L.QE_STAT_REPLY_APP_RESP
    assert L.QE_STAT_READ_RESP == L.QE_STAT_REPLY_HEARTBEAT_RESP
    assert L.QE_STAT_READ_TERM_COMMIT == L.QE_STAT_READY_APPLY


def good():
    """Calls every check passes (G = 4, S = 3, a 16-entry queue)."""
    p = dict(num_groups=4, num_slots=3, inflight_cap=4, stride=4, log_runs=2, read_acks=V,
             read_head=V, read_count=V, read_cap=16, read_ovf=V, read_keys=V, self_slot=V)
    b = {k: V for k in BOOK_FIELDS}
    i = {k: V for k in IN_ROWS}
    o = {k: V for k in RECORD_FIELDS + ("key", "count")}
    o.update(capacity=8)
    return dict(p=p, b=b, i=i, o=o, scratch=V, result=V, ctx=V, index=V, frm=V, null=())


def structs(a):
    i = _lib.QeReadStatesIn(**{k: v for k, v in a["i"].items() if k != "reserved"})
    if "reserved" in a["i"]:
        i.reserved[a["i"]["reserved"]] = 1
    s = dict(p=_lib.QeProgress(**a["p"]), b=_lib.QeReadBook(**a["b"]), i=i,
             o=_lib.QeReadStatesOut(**a["o"]))
    return {k: (None if k in a["null"] else C.byref(v)) for k, v in s.items()}


def call_states(a):
    s = structs(a)
    return _lib.lib().qe_read_states(s["p"], s["b"], s["i"], s["o"], a["scratch"], None, None)


def call_note(a):
    s = structs(a)
    return _lib.lib().qe_read_note(s["p"], s["b"], a["result"], a["ctx"], a["index"], a["frm"],
                                   None)


def upd(part, **kw):
    return lambda a: a[part].update(**kw)


def null(*names):
    return lambda a: a.update(null=names)


STATES_BAD = {
    "NULL p": null("p"), "NULL in": null("i"), "NULL out": null("o"),
    "NULL b with read_released": null("b"),
    "NULL req_index with read_released": upd("b", req_index=None),
    "NULL req_from with read_released": upd("b", req_from=None),
    "NULL read_head": upd("p", read_head=None),
    "NULL read_count": upd("p", read_count=None),
    "term_commit without term_commit_index": upd("i", term_commit_index=None),
    "ri_result without ri_index": upd("i", ri_index=None),
    "in.reserved[0]": upd("i", reserved=0), "in.reserved[1]": upd("i", reserved=1),
    "NULL scratch": lambda a: a.update(scratch=None),
    "scratch not 8-B aligned": lambda a: a.update(scratch=C.c_void_p(68)),
    "NULL count": upd("o", count=None),
    "num_slots 0": upd("p", num_slots=0), "num_slots 17": upd("p", num_slots=17),
    "p.reserved": upd("p", reserved=1), "p.reserved2": upd("p", reserved2=1),
    "p.reserved3": upd("p", reserved3=1),
    "a queue past the word without read_ovf": upd("p", read_ovf=None),
}
for _k in RECORD_FIELDS:
    STATES_BAD[f"capacity > 0 with NULL {_k}"] = upd("o", **{_k: None})


@pytest.mark.parametrize("case", sorted(STATES_BAD))
def test_read_states_einval(case):
    a = good()
    STATES_BAD[case](a)
    assert call_states(a) == _lib.QE_EINVAL, case


def test_read_states_einval_holds_for_an_empty_batch_too():
    """num_groups == 0 skips no check but scratch's."""
    for case in ("NULL count", "NULL b with read_released", "NULL read_head",
                 "capacity > 0 with NULL kind", "ri_result without ri_index", "in.reserved[1]"):
        a = good()
        a["p"].update(num_groups=0, stride=0)
        a["scratch"] = None
        STATES_BAD[case](a)
        assert call_states(a) == _lib.QE_EINVAL, case


def test_read_states_read_cap_out_of_range():
    for cap in (3, 256):
        a = good()
        a["p"].update(read_cap=cap)
        assert call_states(a) == _lib.QE_ERANGE
        assert call_note(a) == _lib.QE_ERANGE


def test_read_states_chunks_past_a_launch():
    """More 4096-group chunks than the 2^31 - 1 blocks of a launch: QE_ERANGE,
    the status qe_ready gives for the same check (the count kernel's grid is one
    block per chunk and would be cut to 32 bits).  It is an argument check: it
    comes before the first HIP call, so the status is neither QE_OK nor QE_EHIP
    whether or not a device is there, and every other argument is good()'s."""
    chunk = 4096
    a = good()
    a["p"].update(num_groups=0x7FFFFFFF * chunk + 1, stride=0x7FFFFFFF * chunk + 1)
    assert call_states(a) == _lib.QE_ERANGE
    # ... and it does not hide the argument errors in front of it
    a["o"].update(count=None)
    assert call_states(a) == _lib.QE_EINVAL


NOTE_BAD = {
    "NULL p": null("p"), "NULL b": null("b"),
    "NULL req_index": upd("b", req_index=None), "NULL req_from": upd("b", req_from=None),
    "NULL result": lambda a: a.update(result=None),
    "NULL ctx": lambda a: a.update(ctx=None),
    "NULL index": lambda a: a.update(index=None),
    "p.reserved3": upd("p", reserved3=1),
}


@pytest.mark.parametrize("case", sorted(NOTE_BAD))
def test_read_note_einval(case):
    a = good()
    NOTE_BAD[case](a)
    assert call_note(a) == _lib.QE_EINVAL, case


def test_read_note_with_nothing_to_do():
    """An empty batch: QE_OK, no kernel; `from` may be NULL."""
    a = good()
    a["p"].update(num_groups=0, stride=0)
    a["frm"] = None
    assert call_note(a) == _lib.QE_OK
