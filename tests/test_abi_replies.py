"""The C surface of qe_replies: symbols, struct layout against the ctypes
mirror, and every QE_EINVAL the header lists.  Validation happens before any
HIP call, so the argument errors need no GPU (the pointers are never read)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from etcd_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "etcd_quorum.h")
V = C.c_void_p(64)  # any non-NULL pointer
IN_FIELDS = ("term", "f_result", "f_from", "f_resp_index", "f_reject_hint", "f_resp_log_term",
             "f_ctx", "s_result", "s_from", "s_resp_index", "v_result", "v_type", "v_from",
             "v_resp_term", "v_req_log_term", "v_req_to", "timeout_now", "reserved")
OUT_FIELDS = ("capacity", "group", "to", "type", "term", "index", "log_term", "hint", "ctx",
              "flags", "count")

LAYOUT_PROG = r"""
#include <stdio.h>
#include <stddef.h>
#include "etcd_quorum.h"
#define F(T, m) printf(#T " " #m " %zu\n", offsetof(T, m));
#define Z(T) printf(#T " sizeof %zu\n", sizeof(T));
int main(void) {
  Z(qe_replies_in) """ + " ".join(f"F(qe_replies_in, {k})" for k in IN_FIELDS) + r"""
  Z(qe_replies_out) """ + " ".join(f"F(qe_replies_out, {k})" for k in OUT_FIELDS) + r"""
  printf("QE_RMSG_BAD %d x\n", QE_RMSG_BAD);
  printf("QE_STAT_REPLY %d %d\n", QE_STAT_REPLY_APP_RESP, QE_STAT_REPLY_HEARTBEAT_RESP);
  printf("QE_STAT_REPLY2 %d %d\n", QE_STAT_REPLY_VOTE_RESP, QE_STAT_REPLY_VOTE_REQ);
  printf("QE_STAT_REPLY3 %d %d\n", QE_STAT_REPLY_TIMEOUT_NOW, QE_STAT_REPLY_BAD);
  printf("QE_STAT_SAME %d %d\n", QE_STAT_REPLY_APP_RESP == QE_STAT_VOTE_WON &&
         QE_STAT_REPLY_HEARTBEAT_RESP == QE_STAT_VOTE_PENDING &&
         QE_STAT_REPLY_VOTE_RESP == QE_STAT_GRANTED, QE_STAT_REPLY_VOTE_REQ == QE_STAT_ELECTIONS &&
         QE_STAT_REPLY_TIMEOUT_NOW == QE_STAT_LEADERS && QE_STAT_REPLY_BAD == QE_STAT_REJECTED);
  return 0;
}
"""
CTYPES = {"qe_replies_in": _lib.QeRepliesIn, "qe_replies_out": _lib.QeRepliesOut}


def test_symbols_and_prototypes():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = set(re.findall(r"\s[TW]\s+(qe_\w+)", out))
    assert {"qe_replies", "qe_replies_scratch_bytes"} <= exported
    assert {"qe_replies", "qe_replies_scratch_bytes"} <= set(_lib.PROTOTYPES)
    L = _lib.lib()
    assert L.qe_abi_version() == 8  # additive: the version stays
    # the scan is qe_collect's: the same chunks, the same scratch
    for G in (0, 1, 4096, 4097, 1 << 24):
        assert L.qe_replies_scratch_bytes(G) == L.qe_collect_scratch_bytes(G)


def test_struct_layout_and_constants_match_header(tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_PROG)
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.dirname(HEADER), str(src), "-o",
                           str(exe)])
    seen, fields = {}, {t: [] for t in CTYPES}
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        t, m, v = line.split()
        if t.startswith("QE_"):
            seen[t] = (m, v)
        elif m == "sizeof":
            assert C.sizeof(CTYPES[t]) == int(v), t
        else:
            assert getattr(CTYPES[t], m).offset == int(v), (t, m)
            fields[t].append(m)
    assert fields["qe_replies_in"] == [k for k, _ in _lib.QeRepliesIn._fields_]
    assert fields["qe_replies_out"] == [k for k, _ in _lib.QeRepliesOut._fields_]
    assert seen["QE_RMSG_BAD"][0] == str(_lib.QE_RMSG_BAD) == "255"
    assert seen["QE_STAT_REPLY"] == (str(_lib.QE_STAT_REPLY_APP_RESP),
                                     str(_lib.QE_STAT_REPLY_HEARTBEAT_RESP))
    assert seen["QE_STAT_REPLY2"] == (str(_lib.QE_STAT_REPLY_VOTE_RESP),
                                      str(_lib.QE_STAT_REPLY_VOTE_REQ))
    assert seen["QE_STAT_REPLY3"] == (str(_lib.QE_STAT_REPLY_TIMEOUT_NOW),
                                      str(_lib.QE_STAT_REPLY_BAD))
    assert seen["QE_STAT_SAME"] == ("1", "1")


def good():
    """A call every check passes (G = 4, S = 3): all four families."""
    p = dict(num_groups=4, num_slots=3, inflight_cap=4, stride=4, last_index=V)
    i = {k: V for k in IN_FIELDS if k != "reserved"}
    o = {k: V for k in OUT_FIELDS if k != "capacity"}
    o["capacity"] = 8
    return p, i, o


def call(p, i, o, scratch=V, null=()):
    L = _lib.lib()
    reserved = i.pop("reserved", None)
    ps, ins, outs = _lib.QeProgress(**p), _lib.QeRepliesIn(**i), _lib.QeRepliesOut(**o)
    if reserved is not None:
        ins.reserved[reserved] = 1
    return L.qe_replies(None if "p" in null else C.byref(ps),
                        None if "in" in null else C.byref(ins),
                        None if "out" in null else C.byref(outs), scratch, None, None)


BAD = {
    "NULL p": lambda p, i, o: dict(null=("p",)),
    "NULL in": lambda p, i, o: dict(null=("in",)),
    "NULL out": lambda p, i, o: dict(null=("out",)),
    "NULL scratch": lambda p, i, o: dict(scratch=None),
    "scratch not 8-B aligned": lambda p, i, o: dict(scratch=C.c_void_p(68)),
    "NULL count": lambda p, i, o: o.update(count=None),
    "NULL term": lambda p, i, o: i.update(term=None),
    "stride < num_groups": lambda p, i, o: p.update(stride=3),
    "num_slots 0": lambda p, i, o: p.update(num_slots=0),
    "num_slots 17": lambda p, i, o: p.update(num_slots=17),
    "in.reserved[0]": lambda p, i, o: i.update(reserved=0),
    "in.reserved[1]": lambda p, i, o: i.update(reserved=1),
    "p.reserved": lambda p, i, o: p.update(reserved=1),
    "p.reserved2": lambda p, i, o: p.update(reserved2=1),
    "p.reserved3": lambda p, i, o: p.update(reserved3=1),
    "v_result without p.last_index": lambda p, i, o: p.update(last_index=None),
}
for _k in ("f_from", "f_resp_index", "f_reject_hint", "f_resp_log_term"):
    BAD[f"f_result without {_k}"] = lambda p, i, o, k=_k: i.update(**{k: None})
for _k in ("s_from", "s_resp_index"):
    BAD[f"s_result without {_k}"] = lambda p, i, o, k=_k: i.update(**{k: None})
for _k in ("v_type", "v_from", "v_resp_term", "v_req_log_term", "v_req_to"):
    BAD[f"v_result without {_k}"] = lambda p, i, o, k=_k: i.update(**{k: None})
for _k in ("group", "to", "type", "term", "index", "log_term", "hint"):
    BAD[f"capacity > 0 with NULL {_k}"] = lambda p, i, o, k=_k: o.update(**{k: None})


@pytest.mark.parametrize("case", sorted(BAD))
def test_einval(case):
    p, i, o = good()
    kw = BAD[case](p, i, o)
    assert call(p, i, o, **(kw if isinstance(kw, dict) else {})) == _lib.QE_EINVAL, case


def test_einval_holds_for_an_empty_batch_too():
    """num_groups == 0 skips no check but scratch's."""
    for upd in (lambda p, i, o: o.update(count=None), lambda p, i, o: i.update(term=None),
                lambda p, i, o: i.update(s_from=None), lambda p, i, o: o.update(hint=None)):
        p, i, o = good()
        p.update(num_groups=0, stride=0)
        upd(p, i, o)
        assert call(p, i, o, scratch=None) == _lib.QE_EINVAL


def check_count_zeroed(p, i, o, scratch):
    """The call is QE_OK with *count = 0.  The zero is a device write: with a
    device it is checked; without one the call still passes every argument
    check (it fails in the runtime, not with QE_EINVAL)."""
    import torch

    if torch.cuda.is_available():
        count = torch.full((1,), 77, dtype=torch.int64, device="cuda")
        o.update(count=C.c_void_p(count.data_ptr()))
        assert call(p, i, o, scratch=scratch) == _lib.QE_OK
        torch.cuda.synchronize()
        assert int(count.item()) == 0
    else:
        host = C.c_uint64(77)
        o.update(count=C.cast(C.pointer(host), C.c_void_p))
        assert call(p, i, o, scratch=scratch) in (_lib.QE_OK, _lib.QE_EHIP)


def test_empty_batch():
    """num_groups == 0 is QE_OK with *count = 0; ctx, flags and (with capacity
    0) every record array may be NULL."""
    p, i, o = good()
    p.update(num_groups=0, stride=0)
    o.update({k: None for k in OUT_FIELDS if k not in ("capacity", "count")}, capacity=0)
    check_count_zeroed(p, i, o, None)


def test_all_families_absent():
    """No result row and no timeout_now: QE_OK with *count = 0, whatever G."""
    p, i, o = good()
    i = dict(term=V)
    p.update(last_index=None)
    o.update(ctx=None, flags=None)
    check_count_zeroed(p, i, o, V)
