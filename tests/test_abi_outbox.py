"""The C surface of qe_outbox: symbols, struct layout against the ctypes
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

LAYOUT_PROG = r"""
#include <stdio.h>
#include <stddef.h>
#include "etcd_quorum.h"
#define F(T, m) printf(#T " " #m " %zu\n", offsetof(T, m));
#define Z(T) printf(#T " sizeof %zu\n", sizeof(T));
int main(void) {
  Z(qe_outbox_in) F(qe_outbox_in, sent) F(qe_outbox_in, snap) F(qe_outbox_in, hb_sent)
  F(qe_outbox_in, index) F(qe_outbox_in, next_before) F(qe_outbox_in, term)
  F(qe_outbox_in, snap_term) F(qe_outbox_in, hb_commit) F(qe_outbox_in, hb_ctx)
  F(qe_outbox_in, max_entries) F(qe_outbox_in, reserved)
  Z(qe_outbox_out) F(qe_outbox_out, capacity) F(qe_outbox_out, msg_runs)
  F(qe_outbox_out, reserved) F(qe_outbox_out, group) F(qe_outbox_out, to)
  F(qe_outbox_out, type) F(qe_outbox_out, term) F(qe_outbox_out, index)
  F(qe_outbox_out, log_term) F(qe_outbox_out, commit) F(qe_outbox_out, ctx)
  F(qe_outbox_out, ent_len) F(qe_outbox_out, ent_term) F(qe_outbox_out, count)
  printf("QE_OMSG %d %d\n", QE_OMSG_APP, QE_OMSG_SNAP);
  printf("QE_OMSG2 %d %d\n", QE_OMSG_HEARTBEAT, QE_OMSG_BAD);
  printf("QE_STAT_OUTBOX %d %d\n", QE_STAT_OUTBOX_ENTRIES, QE_STAT_OUTBOX_APP);
  printf("QE_STAT_OUTBOX2 %d %d\n", QE_STAT_OUTBOX_SNAP, QE_STAT_OUTBOX_HEARTBEAT);
  printf("QE_STAT_OUTBOX_BAD %d x\n", QE_STAT_OUTBOX_BAD);
  return 0;
}
"""
CTYPES = {"qe_outbox_in": _lib.QeOutboxIn, "qe_outbox_out": _lib.QeOutboxOut}


def test_symbols_and_prototypes():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = set(re.findall(r"\s[TW]\s+(qe_\w+)", out))
    assert {"qe_outbox", "qe_outbox_scratch_bytes"} <= exported
    assert {"qe_outbox", "qe_outbox_scratch_bytes"} <= set(_lib.PROTOTYPES)
    L = _lib.lib()
    assert L.qe_abi_version() == 8  # additive: the version stays
    # the scan is qe_collect's: the same chunks, the same scratch
    for G in (0, 1, 4096, 4097, 1 << 24):
        assert L.qe_outbox_scratch_bytes(G) == L.qe_collect_scratch_bytes(G)


def test_struct_layout_and_constants_match_header(tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_PROG)
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.dirname(HEADER), str(src), "-o",
                           str(exe)])
    seen = {}
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        t, m, v = line.split()
        if t.startswith("QE_"):
            seen[t] = (m, v)
        elif m == "sizeof":
            assert C.sizeof(CTYPES[t]) == int(v), t
        else:
            assert getattr(CTYPES[t], m).offset == int(v), (t, m)
    assert seen["QE_OMSG"] == (str(_lib.QE_OMSG_APP), str(_lib.QE_OMSG_SNAP))
    assert seen["QE_OMSG2"] == (str(_lib.QE_OMSG_HEARTBEAT), str(_lib.QE_OMSG_BAD)) == ("3", "255")
    assert seen["QE_STAT_OUTBOX"] == (str(_lib.QE_STAT_OUTBOX_ENTRIES), str(_lib.QE_STAT_OUTBOX_APP))
    assert seen["QE_STAT_OUTBOX2"] == (str(_lib.QE_STAT_OUTBOX_SNAP),
                                       str(_lib.QE_STAT_OUTBOX_HEARTBEAT))
    assert seen["QE_STAT_OUTBOX_BAD"][0] == str(_lib.QE_STAT_OUTBOX_BAD)


def good():
    """A call every check passes (G = 4, S = 3)."""
    p = dict(num_groups=4, num_slots=3, inflight_cap=4, stride=4, log_runs=2, next=V, peer=V,
             committed=V, first_index=V, last_index=V, run_first=V, run_term=V, run_count=V,
             snap_index=V)
    i = dict(sent=V, snap=V, hb_sent=V, index=V, next_before=None, term=V, hb_commit=V)
    o = dict(capacity=8, msg_runs=2, group=V, to=V, type=V, term=V, index=V, log_term=V,
             commit=V, ctx=None, ent_len=V, ent_term=V, count=V)
    return p, i, o


def call(p, i, o, scratch=V, null=()):
    L = _lib.lib()
    ps, ins, outs = _lib.QeProgress(**p), _lib.QeOutboxIn(**i), _lib.QeOutboxOut(**o)
    return L.qe_outbox(None if "p" in null else C.byref(ps), None if "in" in null else C.byref(ins),
                       None if "out" in null else C.byref(outs), scratch, None, None)


BAD = {
    "NULL p": lambda p, i, o: dict(null=("p",)),
    "NULL in": lambda p, i, o: dict(null=("in",)),
    "NULL out": lambda p, i, o: dict(null=("out",)),
    "NULL scratch": lambda p, i, o: dict(scratch=None),
    "scratch not 8-B aligned": lambda p, i, o: dict(scratch=C.c_void_p(68)),
    "NULL count": lambda p, i, o: o.update(count=None),
    "NULL term": lambda p, i, o: i.update(term=None),
    "NULL committed": lambda p, i, o: p.update(committed=None),
    "NULL last_index": lambda p, i, o: p.update(last_index=None),
    "NULL run_first": lambda p, i, o: p.update(run_first=None),
    "NULL run_term": lambda p, i, o: p.update(run_term=None),
    "NULL run_count": lambda p, i, o: p.update(run_count=None),
    "sent with neither index nor next_before": lambda p, i, o: i.update(index=None),
    "next_before used without next": lambda p, i, o: (i.update(index=None, next_before=V),
                                                      p.update(next=None)),
    "next_before used without peer": lambda p, i, o: (i.update(index=None, next_before=V),
                                                      p.update(peer=None)),
    "snap with neither snap_index nor first_index": lambda p, i, o: p.update(snap_index=None,
                                                                             first_index=None),
    "hb_sent without hb_commit": lambda p, i, o: i.update(hb_commit=None),
    "msg_runs > QE_MAX_MSG_RUNS": lambda p, i, o: o.update(msg_runs=5),
    "msg_runs without ent_len": lambda p, i, o: o.update(ent_len=None),
    "msg_runs without ent_term": lambda p, i, o: o.update(ent_term=None),
    "log_runs 0": lambda p, i, o: p.update(log_runs=0),
    "log_runs > QE_MAX_LOG_RUNS": lambda p, i, o: p.update(log_runs=17),
    "stride < num_groups": lambda p, i, o: p.update(stride=3),
    "num_slots 0": lambda p, i, o: p.update(num_slots=0),
    "num_slots 17": lambda p, i, o: p.update(num_slots=17),
    "in.reserved": lambda p, i, o: i.update(reserved=1),
    "out.reserved": lambda p, i, o: o.update(reserved=1),
    "p.reserved": lambda p, i, o: p.update(reserved=1),
    "p.reserved2": lambda p, i, o: p.update(reserved2=1),
    "p.reserved3": lambda p, i, o: p.update(reserved3=1),
}
for _k in ("group", "to", "type", "term", "index", "log_term", "commit"):
    BAD[f"capacity > 0 with NULL {_k}"] = lambda p, i, o, k=_k: o.update(**{k: None})


@pytest.mark.parametrize("case", sorted(BAD))
def test_einval(case):
    p, i, o = good()
    kw = BAD[case](p, i, o)
    assert call(p, i, o, **(kw if isinstance(kw, dict) else {})) == _lib.QE_EINVAL, case


def test_einval_holds_for_an_empty_batch_too():
    """num_groups == 0 skips no check but scratch's."""
    p, i, o = good()
    p.update(num_groups=0, stride=0)
    o.update(count=None)
    assert call(p, i, o, scratch=None) == _lib.QE_EINVAL
    p, i, o = good()
    p.update(num_groups=0, stride=0)
    i.update(term=None)
    assert call(p, i, o, scratch=None) == _lib.QE_EINVAL


def test_empty_batch():
    """num_groups == 0 is QE_OK with *count = 0.  The zero is a device write:
    with a device it is checked; without one the call still passes every
    argument check (it fails in the runtime, not with QE_EINVAL)."""
    import torch

    p, i, o = good()
    p.update(num_groups=0, stride=0)
    o.update(capacity=0, group=None, to=None, type=None, term=None, index=None, log_term=None,
             commit=None, msg_runs=0, ent_len=None, ent_term=None)
    if torch.cuda.is_available():
        count = torch.full((1,), 77, dtype=torch.int64, device="cuda")
        o.update(count=C.c_void_p(count.data_ptr()))
        assert call(p, i, o, scratch=None) == _lib.QE_OK
        torch.cuda.synchronize()
        assert int(count.item()) == 0
    else:
        host = C.c_uint64(77)
        o.update(count=C.cast(C.pointer(host), C.c_void_p))
        assert call(p, i, o, scratch=None) in (_lib.QE_OK, _lib.QE_EHIP)
