"""The C surface of qe_apply_conf: symbols, struct layout against the ctypes
mirror, every QE_AC_* constant and every QE_EINVAL the header lists.
Validation happens before any HIP call, so the argument errors need no GPU (the
pointers are never read)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from etcd_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "etcd_quorum.h")
V = C.c_void_p(64)  # any non-NULL pointer, 16-B aligned
IN_FIELDS = ("capacity", "n", "count", "max_changes", "reserved", "group", "transition",
             "num_changes", "type", "node_id", "slot")
OUT_REQUIRED = ("result", "cc_result", "sw_result", "inc", "out", "learner", "learners_next",
                "tracked", "new_progress", "auto_leave")
OUT_FIELDS = OUT_REQUIRED + ("ids",)
CONF_ROWS = ("slot_ids", "inc_mask", "out_mask", "learner_mask", "learners_next_mask",
             "is_learner", "tracked", "auto_leave")
PROGRESS_ROWS = ("match", "next", "pending_snapshot", "peer", "infl_lo", "infl_hi", "committed",
                 "term_start", "first_index", "last_index")
STRUCTS = {"qe_apply_conf_in": (IN_FIELDS, _lib.QeApplyConfIn),
           "qe_apply_conf_out": (OUT_FIELDS, _lib.QeApplyConfOut)}
AC_NAMES = ("QE_AC_AUTO", "QE_AC_JOINT_IMPLICIT", "QE_AC_JOINT_EXPLICIT", "QE_AC_ANY_SLOT",
            "QE_AC_APPLIED", "QE_AC_LEADER", "QE_AC_DEFERRED", "QE_AC_REFUSED", "QE_AC_BAD_GROUP",
            "QE_AC_BAD_ORDER", "QE_AC_BAD_CHANGE", "QE_AC_CHANGER_ERROR", "QE_AC_SKIPPED")
CC_NAMES = ("QE_CC_OK", "QE_CC_ERR_INVARIANT", "QE_CC_ERR_ALREADY_JOINT",
            "QE_CC_ERR_ZERO_VOTER_JOINT", "QE_CC_ERR_NOT_JOINT", "QE_CC_ERR_SIMPLE_IN_JOINT",
            "QE_CC_ERR_BAD_TYPE", "QE_CC_ERR_REMOVED_ALL", "QE_CC_ERR_SIMPLE_MULTI",
            "QE_CC_ERR_INVARIANT_OUT", "QE_CC_ERR_NO_SLOT")

LAYOUT_PROG = r"""
#include <stdio.h>
#include <stddef.h>
#include "etcd_quorum.h"
#define F(T, m) printf(#T " " #m " %zu\n", offsetof(T, m));
#define Z(T) printf(#T " sizeof %zu\n", sizeof(T));
#define K(c) printf("const " #c " %d\n", (int)(c));
int main(void) {
""" + "\n".join(f"  Z({t}) " + " ".join(f"F({t}, {k})" for k in fs)
                for t, (fs, _) in STRUCTS.items()) + "\n" + "\n".join(
                    f"  K({c})" for c in AC_NAMES + CC_NAMES) + r"""
  return 0;
}
"""
NAMES = {"qe_apply_conf", "qe_apply_conf_scratch_bytes"}


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
    # two byte rows per group (switched, the switch results), each padded to 16 B
    for G in (0, 1, 16, 17, 135, 1 << 24):
        assert 2 * G <= L.qe_apply_conf_scratch_bytes(G) <= 2 * G + 32
        assert L.qe_apply_conf_scratch_bytes(G) % 16 == 0


def test_struct_layout_and_constants_match_header(tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_PROG)
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.dirname(HEADER), str(src), "-o",
                           str(exe)])
    consts, fields = {}, {t: [] for t in STRUCTS}
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        t, m, v = line.split()
        if t == "const":
            consts[m] = int(v)
        elif m == "sizeof":
            assert C.sizeof(STRUCTS[t][1]) == int(v), t
        else:
            assert getattr(STRUCTS[t][1], m).offset == int(v), (t, m)
            fields[t].append(m)
    for t, (fs, ct) in STRUCTS.items():
        assert fields[t] == list(fs) == [k for k, _ in ct._fields_], t
    assert set(consts) == set(AC_NAMES + CC_NAMES)
    for name, v in consts.items():
        assert getattr(_lib, name) == v, name
    # every QE_AC_* the header defines is checked here
    with open(HEADER, encoding="utf-8") as f:
        assert set(re.findall(r"^#define (QE_AC_\w+)", f.read(), re.M)) == set(AC_NAMES)
    # refusals are the codes >= QE_AC_REFUSED, and only they
    refusals = {"QE_AC_BAD_GROUP", "QE_AC_BAD_ORDER", "QE_AC_BAD_CHANGE", "QE_AC_CHANGER_ERROR",
                "QE_AC_SKIPPED"}
    for name in ("QE_AC_APPLIED", "QE_AC_LEADER", "QE_AC_DEFERRED") + tuple(refusals):
        assert (consts[name] >= consts["QE_AC_REFUSED"]) == (name in refusals), name
    assert len({consts[k] for k in AC_NAMES[4:7] + tuple(refusals)}) == 8


def good():
    """A call every check passes (G = 4, S = 3, F = 4, R = 2, capacity 8, C = 2)."""
    p = dict(num_groups=4, num_slots=3, inflight_cap=4, stride=4, log_runs=2,
             run_first=V, run_term=V, run_count=V, inc_mask=V, out_mask=V, tracked=V, self_slot=V,
             **{k: V for k in PROGRESS_ROWS})
    f = dict(term=V, state=V, lead=V, vote=V)
    c = dict(num_groups=4, num_slots=3, **{k: V for k in CONF_ROWS})
    i = dict(capacity=8, n=3, max_changes=2, group=V, transition=V, num_changes=V, type=V,
             node_id=V, slot=V)
    o = {k: V for k in OUT_FIELDS}
    sw = dict(result=V, sent=V, snap=V)
    return dict(p=p, f=f, c=c, i=i, o=o, sw=sw, scratch=V, null=())


def call(a):
    s = dict(p=_lib.QeProgress(**a["p"]), f=_lib.QeFollower(**a["f"]), c=_lib.QeConf(**a["c"]),
             i=_lib.QeApplyConfIn(**a["i"]), o=_lib.QeApplyConfOut(**a["o"]),
             sw=_lib.QeSwitch(**a["sw"]))
    s = {k: (None if k in a["null"] else C.byref(v)) for k, v in s.items()}
    return _lib.lib().qe_apply_conf(s["p"], s["f"], s["c"], s["i"], s["o"], s["sw"], a["scratch"],
                                    None)


def upd(part, **kw):
    return lambda a: a[part].update(**kw)


def null(*names):
    return lambda a: a.update(null=names)


BAD = {
    "NULL p": null("p"), "NULL f": null("f"), "NULL c": null("c"), "NULL in": null("i"),
    "NULL out": null("o"),
    "NULL scratch": lambda a: a.update(scratch=None),
    "scratch not 16-B aligned": lambda a: a.update(scratch=C.c_void_p(72)),
    # what qe_switch_config refuses in p
    "num_slots 0": upd("p", num_slots=0), "num_slots 17": upd("p", num_slots=17),
    "p.reserved": upd("p", reserved=1), "p.reserved2": upd("p", reserved2=1),
    "p.reserved3": upd("p", reserved3=1),
    "stride < num_groups": upd("p", stride=3),
    "log_runs > 0 with NULL run_first": upd("p", run_first=None),
    "NULL f.state": upd("f", state=None),
    "NULL p.inc_mask": upd("p", inc_mask=None), "NULL p.out_mask": upd("p", out_mask=None),
    "NULL p.tracked": upd("p", tracked=None), "NULL p.self_slot": upd("p", self_slot=None),
    "c.num_groups differs": upd("c", num_groups=5), "c.num_slots differs": upd("c", num_slots=4),
    "c.reserved": upd("c", reserved=1),
    "in.reserved": upd("i", reserved=1), "max_changes 256": upd("i", max_changes=256),
    "max_changes > 0 with NULL type": upd("i", type=None),
    "max_changes > 0 with NULL node_id": upd("i", node_id=None),
    "sw with NULL result": upd("sw", result=None),
    "sw with bytes_requested": upd("sw", bytes_requested=V),
}
for _k in PROGRESS_ROWS:
    BAD[f"NULL p.{_k}"] = upd("p", **{_k: None})
for _k in CONF_ROWS:
    BAD[f"NULL c.{_k}"] = upd("c", **{_k: None})
for _k in ("group", "transition", "num_changes"):
    BAD[f"capacity > 0 with NULL in.{_k}"] = upd("i", **{_k: None})
for _k in OUT_REQUIRED:
    BAD[f"capacity > 0 with NULL out.{_k}"] = upd("o", **{_k: None})


@pytest.mark.parametrize("case", sorted(BAD))
def test_einval(case):
    a = good()
    BAD[case](a)
    assert call(a) == _lib.QE_EINVAL, case


def test_erange_of_the_switch_kernel_stays_erange():
    for kw in (dict(inflight_cap=0), dict(inflight_cap=256), dict(log_runs=17)):
        a = good()
        a["p"].update(**kw)
        assert call(a) == _lib.QE_ERANGE, kw


def test_einval_holds_with_nothing_to_do_too():
    """capacity == 0 and num_groups == 0 skip no check but the list's arrays."""
    for case in ("NULL f.state", "NULL c.tracked", "in.reserved", "NULL scratch",
                 "sw with NULL result", "NULL p.self_slot"):
        a = good()
        a["i"].update(capacity=0)
        BAD[case](a)
        assert call(a) == _lib.QE_EINVAL, case


def test_nothing_to_do():
    """capacity == 0 (every list and output array may be NULL, sw too) or an
    empty batch: QE_OK, no kernel."""
    a = good()
    a["i"] = dict(capacity=0, n=5)
    a["o"] = {}
    a["null"] = ("sw",)
    assert call(a) == _lib.QE_OK
    a = good()
    a["p"].update(num_groups=0, stride=0)
    a["c"].update(num_groups=0)
    assert call(a) == _lib.QE_OK

