"""The C surface of qe_carry: symbols, struct layout against the ctypes mirror,
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

FIELDS = {"qe_peers": [f for f, _ in _lib.QePeers._fields_],
          "qe_carry_in": [f for f, _ in _lib.QeCarryIn._fields_],
          "qe_carry_out": [f for f, _ in _lib.QeCarryOut._fields_]}
CTYPES = {"qe_peers": _lib.QePeers, "qe_carry_in": _lib.QeCarryIn, "qe_carry_out": _lib.QeCarryOut}
CONSTANTS = ["QE_PEER_NONE", "QE_CARRY_SNAP_STATUS", "QE_CARRY_TYPES", "QE_TD_LOCAL",
             "QE_TD_REMOTE", "QE_TD_LOST", "QE_TD_BAD", "QE_STAT_CARRY_LOCAL",
             "QE_STAT_CARRY_REMOTE", "QE_STAT_CARRY_LOST", "QE_STAT_CARRY_BAD",
             "QE_STAT_CARRY_SNAP_STATUS"]
LAYOUT_PROG = r"""
#include <stdio.h>
#include <stddef.h>
#include "etcd_quorum.h"
#define F(T, m) printf(#T " " #m " %zu\n", offsetof(T, m));
#define Z(T) printf(#T " sizeof %zu\n", sizeof(T));
#define K(c) printf(#c " value %llu\n", (unsigned long long)(c));
int main(void) {
  Z(qe_peers) Z(qe_carry_in) Z(qe_carry_out)
""" + "\n".join(f"  F({t}, {'from' if f == 'from_' else f})" for t, fs in FIELDS.items()
                for f in fs) + "\n" + \
    "\n".join(f"  K({c})" for c in CONSTANTS) + "\n  return 0;\n}\n"


def test_symbols_and_prototypes():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = set(re.findall(r"\s[TW]\s+(qe_\w+)", out))
    assert {"qe_carry", "qe_carry_scratch_bytes"} <= exported
    assert {"qe_carry", "qe_carry_scratch_bytes"} <= set(_lib.PROTOTYPES)
    assert _lib.lib().qe_abi_version() == 8  # additive: the version stays


def test_scratch_size_formula():
    """Two bytes per record and the two collect scratches: nothing G-sized."""
    L = _lib.lib()
    assert L.qe_carry_scratch_bytes(0) == 2 * L.qe_collect_scratch_bytes(0) == 128
    for n in (1, 4096, 4097, 1 << 24, 0xFFFFFFF0):
        assert L.qe_carry_scratch_bytes(n) == 2 * n + 2 * L.qe_collect_scratch_bytes(n), n


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
    assert seen["QE_PEER_NONE"] == (1 << 64) - 1 and seen["QE_TD_BAD"] == 255
    assert seen["QE_CARRY_TYPES"] == sum(1 << t for t in list(range(1, 7)) + list(range(10, 16)))
    assert sorted(seen[c] for c in CONSTANTS[3:6]) == [1, 2, 3]
    stats = [seen[c] for c in CONSTANTS if c.startswith("QE_STAT_CARRY")]
    assert len(set(stats) | {0, 14, 15}) == len(stats) + 3  # no counter is shared
    assert seen["QE_STAT_CARRY_BAD"] == _lib.QE_STAT_INBOX_BAD


OPTIONAL_IN = ("commit", "hint", "ctx", "mflags", "drop", "cut")
OPTIONAL_OUT = ("ctx", "mflags", "src")


def good():
    """A call every check passes (G = 4, S = 3, capacity 8 -> 16, E 2 -> 3)."""
    p = dict(num_groups=4, num_slots=3, stride=4)
    pe = dict(peer_group=V, peer_from=V)
    i = {k: (None if k in OPTIONAL_IN else V) for k in FIELDS["qe_carry_in"]}
    i.update(capacity=8, msg_runs=2, flags=_lib.QE_CARRY_SNAP_STATUS, ignore=1 << 6, reserved=0)
    o = {k: (None if k in OPTIONAL_OUT else V) for k in FIELDS["qe_carry_out"]}
    o.update(capacity=16, base=3, ent_pitch=16, msg_runs=3, reserved=0)
    return p, pe, i, o


def call(p, pe, i, o, scratch=V, null=()):
    L = _lib.lib()
    ps, pes = _lib.QeProgress(**p), _lib.QePeers(**pe)
    ins, outs = _lib.QeCarryIn(**i), _lib.QeCarryOut(**o)
    arg = lambda name, s: None if name in null else C.byref(s)  # noqa: E731
    return L.qe_carry(arg("p", ps), arg("peers", pes), arg("in", ins), arg("out", outs), scratch,
                      None, None)


BAD = {
    "NULL p": lambda p, pe, i, o: dict(null=("p",)),
    "NULL peers": lambda p, pe, i, o: dict(null=("peers",)),
    "NULL in": lambda p, pe, i, o: dict(null=("in",)),
    "NULL out": lambda p, pe, i, o: dict(null=("out",)),
    "NULL scratch": lambda p, pe, i, o: dict(scratch=None),
    "scratch not 8-B aligned": lambda p, pe, i, o: dict(scratch=C.c_void_p(68)),
    "NULL peer_group": lambda p, pe, i, o: pe.update(peer_group=None),
    "NULL peer_from": lambda p, pe, i, o: pe.update(peer_from=None),
    "E_in > E_out": lambda p, pe, i, o: i.update(msg_runs=4),
    "E_out > QE_MAX_MSG_RUNS": lambda p, pe, i, o: o.update(msg_runs=5),
    "E_in > QE_MAX_MSG_RUNS": lambda p, pe, i, o: (i.update(msg_runs=5), o.update(msg_runs=5)),
    "E_in without in.ent_len": lambda p, pe, i, o: i.update(ent_len=None),
    "E_in without in.ent_term": lambda p, pe, i, o: i.update(ent_term=None),
    "E_out without out.ent_len": lambda p, pe, i, o: o.update(ent_len=None),
    "E_out without out.ent_term": lambda p, pe, i, o: o.update(ent_term=None),
    "base > capacity": lambda p, pe, i, o: o.update(base=17),
    "ent_pitch < capacity": lambda p, pe, i, o: o.update(ent_pitch=15),
    "in.reserved": lambda p, pe, i, o: i.update(reserved=1),
    "out.reserved": lambda p, pe, i, o: o.update(reserved=1),
    "p.reserved": lambda p, pe, i, o: p.update(reserved=1),
    "p.reserved2": lambda p, pe, i, o: p.update(reserved2=1),
    "num_slots 0": lambda p, pe, i, o: p.update(num_slots=0),
    "num_slots 17": lambda p, pe, i, o: p.update(num_slots=17),
    "stride < num_groups": lambda p, pe, i, o: p.update(stride=3),
    "unknown flags": lambda p, pe, i, o: i.update(flags=2),
}
for _t in (0, 7, 8, 9, 16, 31):
    BAD[f"ignore bit {_t}"] = lambda p, pe, i, o, t=_t: i.update(ignore=1 << t)
for _k in ("count", "group", "to", "type", "term", "index", "log_term"):
    BAD[f"NULL in.{_k}"] = lambda p, pe, i, o, k=_k: i.update(**{k: None})
for _k in ("group", "from_", "type", "term", "index", "log_term", "commit", "hint", "count",
           "disposition", "remote", "remote_count"):
    BAD[f"NULL out.{_k}"] = lambda p, pe, i, o, k=_k: o.update(**{k: None})


@pytest.mark.parametrize("case", sorted(BAD))
def test_einval(case):
    p, pe, i, o = good()
    kw = BAD[case](p, pe, i, o)
    assert call(p, pe, i, o, **(kw if isinstance(kw, dict) else {})) == _lib.QE_EINVAL, case


def test_erange():
    """Positions are 32 bits: a capacity above 0xFFFFFFF0."""
    p, pe, i, o = good()
    i.update(capacity=0xFFFFFFF1)
    assert call(p, pe, i, o) == _lib.QE_ERANGE


def test_einval_holds_for_an_empty_list():
    """capacity == 0 needs no record array and no scratch, and skips no other check."""
    for field in ("count", "remote_count"):
        p, pe, i, o = good()
        i.update(capacity=0, group=None, to=None, type=None, term=None, index=None, log_term=None)
        o.update(disposition=None, remote=None, **{field: None})
        assert call(p, pe, i, o, scratch=None) == _lib.QE_EINVAL, field
    p, pe, i, o = good()
    i.update(capacity=0, count=None)
    assert call(p, pe, i, o, scratch=None) == _lib.QE_EINVAL


def test_empty_list():
    """capacity == 0 is QE_OK with both counts 0.  The zeros are device writes: with a device
    they are checked; without one the call still passes every argument check."""
    import torch

    p, pe, i, o = good()
    i.update(capacity=0, group=None, to=None, type=None, term=None, index=None, log_term=None)
    o.update(disposition=None, remote=None)
    if torch.cuda.is_available():
        counts = torch.full((2,), 77, dtype=torch.int64, device="cuda")
        o.update(count=C.c_void_p(counts.data_ptr()), remote_count=C.c_void_p(counts.data_ptr() + 8))
        assert call(p, pe, i, o, scratch=None) == _lib.QE_OK
        torch.cuda.synchronize()
        assert counts.tolist() == [0, 0]
    else:
        host = (C.c_uint64 * 2)(77, 77)
        o.update(count=C.cast(host, C.c_void_p),
                 remote_count=C.c_void_p(C.addressof(host) + 8))
        assert call(p, pe, i, o, scratch=None) in (_lib.QE_OK, _lib.QE_EHIP)
