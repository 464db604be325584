"""The C surface of qe_ready_note / qe_ready / qe_advance: symbols, struct layout
against the ctypes mirror, and every QE_EINVAL the header lists.  Validation
happens before any HIP call, so the argument errors need no GPU (the pointers
are never read)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from etcd_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "etcd_quorum.h")
V = C.c_void_p(64)  # any non-NULL pointer
STATE_FIELDS = ("stable", "applied", "snap_pending", "prev_term", "prev_commit", "prev_vote",
                "prev_lead", "prev_state")
NOTE_FIELDS = ("follow_result", "append_from", "snap_result", "snap_resp_index")
IN_FIELDS = ("pending", "max_apply", "reserved")
RECORD_FIELDS = ("group", "term", "commit", "vote", "lead", "state", "flags", "ent_first",
                 "ent_count", "ent_last_term", "apply_first", "apply_count", "snap_index")
RUN_FIELDS = ("ent_len", "ent_term", "apply_len", "apply_term")
OUT_FIELDS = ("capacity", "ent_runs", "reserved") + RECORD_FIELDS + RUN_FIELDS + ("count",)
OPT_FIELDS = ("auto_leave", "pending_conf_index", "reserved")
LOG_ROWS = ("committed", "last_index", "run_first", "run_term", "run_count")
STRUCTS = {"qe_ready_state": (STATE_FIELDS, _lib.QeReadyState),
           "qe_ready_note_in": (NOTE_FIELDS, _lib.QeReadyNoteIn),
           "qe_ready_in": (IN_FIELDS, _lib.QeReadyIn),
           "qe_ready_out": (OUT_FIELDS, _lib.QeReadyOut),
           "qe_advance_opt": (OPT_FIELDS, _lib.QeAdvanceOpt)}

LAYOUT_PROG = r"""
#include <stdio.h>
#include <stddef.h>
#include "etcd_quorum.h"
#define F(T, m) printf(#T " " #m " %zu\n", offsetof(T, m));
#define Z(T) printf(#T " sizeof %zu\n", sizeof(T));
int main(void) {
""" + "\n".join(f"  Z({t}) " + " ".join(f"F({t}, {k})" for k in fs)
                for t, (fs, _) in STRUCTS.items()) + r"""
  printf("QE_RD %u %u\n", QE_RD_SOFT | QE_RD_HARD << 8 | QE_RD_MUST_SYNC << 16,
         QE_RD_SNAP | QE_RD_ENTS_CUT << 8 | QE_RD_APPLY_CUT << 16);
  printf("QE_ADV %d %d\n", QE_ADV_OK | QE_ADV_OK_STALE_ENTRIES << 8 | QE_ADV_REFUSED << 16,
         QE_ADV_BAD_GROUP | QE_ADV_APPLIED_RANGE << 8);
  printf("QE_ADV2 %u %u\n", QE_ADV_OUTCOME, QE_ADV_AUTO_LEAVE);
  printf("QE_STAT_READY %d %d\n", QE_STAT_READY_ENTRIES | QE_STAT_READY_APPLY << 8,
         QE_STAT_READY_MUST_SYNC);
  printf("QE_STAT_SAME %d %d\n", QE_STAT_READY_ENTRIES == QE_STAT_COMMIT_SUM &&
         QE_STAT_READY_APPLY == QE_STAT_COMMIT_ADVANCED,
         QE_STAT_READY_MUST_SYNC == QE_STAT_VOTE_WON);
  return 0;
}
"""
NAMES = {"qe_ready_note", "qe_ready", "qe_ready_scratch_bytes", "qe_advance"}


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
    # qe_collect's part, then a flag byte per group from a 16-B boundary on
    for G in (0, 1, 4096, 4097, 1 << 24):
        assert L.qe_ready_scratch_bytes(G) >= L.qe_collect_scratch_bytes(G) + G + 15
        assert L.qe_ready_scratch_bytes(G) <= L.qe_collect_scratch_bytes(G) + G + 48


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
    assert seen["QE_RD"] == (L.QE_RD_SOFT | L.QE_RD_HARD << 8 | L.QE_RD_MUST_SYNC << 16,
                             L.QE_RD_SNAP | L.QE_RD_ENTS_CUT << 8 | L.QE_RD_APPLY_CUT << 16)
    assert seen["QE_ADV"] == (L.QE_ADV_OK | L.QE_ADV_OK_STALE_ENTRIES << 8 | L.QE_ADV_REFUSED << 16,
                              L.QE_ADV_BAD_GROUP | L.QE_ADV_APPLIED_RANGE << 8)
    assert seen["QE_ADV2"] == (L.QE_ADV_OUTCOME, L.QE_ADV_AUTO_LEAVE)
    assert seen["QE_STAT_READY"] == (L.QE_STAT_READY_ENTRIES | L.QE_STAT_READY_APPLY << 8,
                                     L.QE_STAT_READY_MUST_SYNC)
    assert seen["QE_STAT_SAME"] == (1, 1)


def good():
    """Calls every check passes (G = 4, S = 3, R = 2, E = 2)."""
    p = dict(num_groups=4, num_slots=3, inflight_cap=4, stride=4, log_runs=2,
             **{k: V for k in LOG_ROWS})
    f = dict(term=V, state=V, lead=V, vote=V)
    rs = {k: V for k in STATE_FIELDS}
    note = {k: V for k in NOTE_FIELDS}
    i = dict(pending=V, max_apply=3)
    o = {k: V for k in RECORD_FIELDS + RUN_FIELDS + ("count",)}
    o.update(capacity=8, ent_runs=2)
    opt = dict(auto_leave=V, pending_conf_index=V)
    return dict(p=p, f=f, rs=rs, note=note, i=i, o=o, opt=opt, scratch=V, result=V, null=())


def structs(a):
    opt = _lib.QeAdvanceOpt(auto_leave=a["opt"].get("auto_leave"),
                            pending_conf_index=a["opt"].get("pending_conf_index"))
    if "reserved" in a["opt"]:
        opt.reserved[a["opt"]["reserved"]] = 1
    s = dict(p=_lib.QeProgress(**a["p"]), f=_lib.QeFollower(**a["f"]),
             rs=_lib.QeReadyState(**a["rs"]), note=_lib.QeReadyNoteIn(**a["note"]),
             i=_lib.QeReadyIn(**a["i"]), o=_lib.QeReadyOut(**a["o"]), opt=opt)
    return {k: (None if k in a["null"] else C.byref(v)) for k, v in s.items()}


def call_note(a):
    s = structs(a)
    return _lib.lib().qe_ready_note(s["p"], s["rs"], s["note"], None)


def call_ready(a):
    s = structs(a)
    return _lib.lib().qe_ready(s["p"], s["f"], s["rs"], s["i"], s["o"], a["scratch"], None, None)


def call_advance(a):
    s = structs(a)
    return _lib.lib().qe_advance(s["p"], s["f"], s["rs"], s["o"], s["opt"], a["result"], None)


def upd(part, **kw):
    return lambda a: a[part].update(**kw)


def null(*names):
    return lambda a: a.update(null=names)


# ---- qe_ready ----
READY_BAD = {
    "NULL p": null("p"), "NULL f": null("f"), "NULL rs": null("rs"), "NULL in": null("i"),
    "NULL out": null("o"),
    "NULL scratch": lambda a: a.update(scratch=None),
    "scratch not 8-B aligned": lambda a: a.update(scratch=C.c_void_p(68)),
    "NULL count": upd("o", count=None),
    "stride < num_groups": upd("p", stride=3),
    "num_slots 0": upd("p", num_slots=0), "num_slots 17": upd("p", num_slots=17),
    "log_runs 0": upd("p", log_runs=0), "log_runs 17": upd("p", log_runs=17),
    "ent_runs 5": upd("o", ent_runs=5),
    "in.reserved": upd("i", reserved=1), "out.reserved": upd("o", reserved=1),
    "p.reserved": upd("p", reserved=1), "p.reserved2": upd("p", reserved2=1),
    "p.reserved3": upd("p", reserved3=1),
}
for _k in LOG_ROWS:
    READY_BAD[f"NULL p.{_k}"] = upd("p", **{_k: None})
for _k in ("term", "state", "lead"):
    READY_BAD[f"NULL f.{_k}"] = upd("f", **{_k: None})
for _k in STATE_FIELDS:
    READY_BAD[f"NULL rs.{_k}"] = upd("rs", **{_k: None})
for _k in RUN_FIELDS:
    READY_BAD[f"ent_runs > 0 with NULL {_k}"] = upd("o", **{_k: None})
for _k in RECORD_FIELDS:
    READY_BAD[f"capacity > 0 with NULL {_k}"] = upd("o", **{_k: None})


@pytest.mark.parametrize("case", sorted(READY_BAD))
def test_ready_einval(case):
    a = good()
    READY_BAD[case](a)
    assert call_ready(a) == _lib.QE_EINVAL, case


def test_ready_einval_holds_for_an_empty_batch_too():
    """num_groups == 0 skips no check but scratch's."""
    for case in ("NULL count", "NULL rs.stable", "capacity > 0 with NULL flags", "ent_runs 5",
                 "NULL f.lead", "in.reserved"):
        a = good()
        a["p"].update(num_groups=0, stride=0)
        a["scratch"] = None
        READY_BAD[case](a)
        assert call_ready(a) == _lib.QE_EINVAL, case


def test_ready_empty_batch():
    """num_groups == 0 is QE_OK with *count = 0; vote, pending and (with
    capacity 0 and ent_runs 0) every record array may be NULL.  The zero is a
    device write: with a device it is checked; without one the call still
    passes every argument check (it fails in the runtime, not with QE_EINVAL)."""
    import torch

    a = good()
    a["p"].update(num_groups=0, stride=0)
    a["f"].update(vote=None)
    a["i"].update(pending=None)
    a["o"] = dict(capacity=0, ent_runs=0)
    a["scratch"] = None
    if torch.cuda.is_available():
        count = torch.full((1,), 77, dtype=torch.int64, device="cuda")
        a["o"].update(count=C.c_void_p(count.data_ptr()))
        assert call_ready(a) == _lib.QE_OK
        torch.cuda.synchronize()
        assert int(count.item()) == 0
    else:
        host = C.c_uint64(77)
        a["o"].update(count=C.cast(C.pointer(host), C.c_void_p))
        assert call_ready(a) in (_lib.QE_OK, _lib.QE_EHIP)


# ---- qe_ready_note ----
NOTE_BAD = {
    "NULL p": null("p"), "NULL rs": null("rs"), "NULL in": null("note"),
    "NULL stable": upd("rs", stable=None),
    "follow_result without append_from": upd("note", append_from=None),
    "append_from without follow_result": upd("note", follow_result=None),
    "snap_result without snap_resp_index": upd("note", snap_resp_index=None),
    "snap_resp_index without snap_result": upd("note", snap_result=None),
    "snap_result with a NULL snap_pending": upd("rs", snap_pending=None),
}


@pytest.mark.parametrize("case", sorted(NOTE_BAD))
def test_note_einval(case):
    a = good()
    NOTE_BAD[case](a)
    assert call_note(a) == _lib.QE_EINVAL, case


def test_note_with_nothing_to_do():
    """Both pairs absent, or an empty batch: QE_OK, no kernel."""
    a = good()
    a["note"] = {}
    assert call_note(a) == _lib.QE_OK
    a = good()
    a["p"].update(num_groups=0, stride=0)
    assert call_note(a) == _lib.QE_OK


# ---- qe_advance ----
ADVANCE_BAD = {
    "NULL p": null("p"), "NULL rs": null("rs"), "NULL list": null("o"),
    "NULL count": upd("o", count=None),
    "NULL result": lambda a: a.update(result=None),
    "stride < num_groups": upd("p", stride=3),
    "num_slots 0": upd("p", num_slots=0),
    "log_runs 0": upd("p", log_runs=0), "log_runs 17": upd("p", log_runs=17),
    "list.reserved": upd("o", reserved=1), "p.reserved3": upd("p", reserved3=1),
    "opt.reserved[0]": upd("opt", reserved=0), "opt.reserved[1]": upd("opt", reserved=1),
    "auto_leave without pending_conf_index": upd("opt", pending_conf_index=None),
    "auto_leave without f": null("f"),
    "auto_leave without f.state": upd("f", state=None),
}
for _k in LOG_ROWS:
    ADVANCE_BAD[f"NULL p.{_k}"] = upd("p", **{_k: None})
for _k in STATE_FIELDS:
    ADVANCE_BAD[f"NULL rs.{_k}"] = upd("rs", **{_k: None})
for _k in RECORD_FIELDS:
    ADVANCE_BAD[f"capacity > 0 with NULL {_k}"] = upd("o", **{_k: None})


@pytest.mark.parametrize("case", sorted(ADVANCE_BAD))
def test_advance_einval(case):
    a = good()
    ADVANCE_BAD[case](a)
    assert call_advance(a) == _lib.QE_EINVAL, case


def test_advance_with_nothing_to_do():
    """capacity 0 (every list array may be NULL, f and opt too) or an empty
    batch: QE_OK, no kernel.  The run arrays are never needed."""
    a = good()
    a["o"] = dict(capacity=0, count=V)
    a["null"] = ("f", "opt")
    assert call_advance(a) == _lib.QE_OK
    a = good()
    a["p"].update(num_groups=0, stride=0)
    a["o"].update({k: None for k in RUN_FIELDS}, ent_runs=0)
    assert call_advance(a) == _lib.QE_OK
