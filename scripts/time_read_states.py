#!/usr/bin/env python3
"""qe_read_states at 16M groups (S = 5, a 16-entry queue, keys tracked), at two
densities: one group in 64 released a request in the step just run, and every
group did (one request each).  The call is its three kernels (count, scan,
fill); device events around one C call with its structs built beforehand,
medians of K runs after warm-up, with the minimum and the maximum.  The window
still holds the host's enqueue of the three launches, as qe_collect's does.

The yardstick is qe_collect over the same flag row (read_released as the
flags, `committed` as the value), timed in the same process and interleaved
with qe_read_states call by call: it is the list primitive the record-list
layer was built from, with the same three passes and fewer bytes per record
(16 against 30 written, and no book to look up).

  python scripts/time_read_states.py [--groups N] [--runs K] [--out FILE]

Prints one JSON document; --out also writes it to a file."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # the MI355X spec sheet: 8.0 TB/s
S, CAP = 5, 16


def algorithmic_bytes(G, records):
    """Per group the released count, 1 B (term_commit and ri_result are not
    given).  Per group with a record: read_head 4 + self_slot 1.  Per record:
    the book's index 8 + origin 1 and the key 8 read, 30 written (group 8, kind
    1, to 1, ctx 4, index 8, key 8)."""
    return G + records * (5 + 17 + 30)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=1 << 24)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("time_read_states: no GPU (there is no CPU fallback to time)")
    from types import SimpleNamespace

    from etcd_amd import engine as e

    dev, G = "cuda:0", a.groups
    i64 = torch.int64
    ps = e.ProgressState(G, S, 4, 1, dev, extras=("self_slot", "reads", "read_keys"), read_cap=CAP)
    g = torch.arange(G, device=dev, dtype=i64)
    ps.self_slot.copy_((g % S).to(torch.uint8))
    ps.read_head.copy_((1000 + g % 977).to(torch.int32))
    ps.committed.copy_(5000 + g % 13)
    ps.read_keys.copy_(torch.arange(G * CAP, device=dev, dtype=i64) * 7919)
    book = e.ReadBook(ps)
    book.req_index.copy_(4000 + torch.arange(G * CAP, device=dev, dtype=i64) % 1000)
    book.req_from.copy_((torch.arange(G * CAP, device=dev, dtype=i64) % (S + 2)).to(torch.uint8))
    gen = torch.Generator(device=dev).manual_seed(7)
    one_in_64 = (torch.rand(G, device=dev, generator=gen) < 1.0 / 64).to(torch.uint8)
    scratch = torch.empty((e._lib.lib().qe_collect_scratch_bytes(G) + 7) // 8, dtype=i64,
                          device=dev)

    def event_ms(f):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        f()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1)

    def summary(ts):
        return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}

    res = {"groups": G, "slots": S, "read_cap": CAP, "runs": a.runs, "hbm_peak_GBs": HBM_PEAK_GBS,
           "densities": {}}
    for name, rel in (("one_in_64", one_in_64), ("every_group", torch.ones_like(one_in_64))):
        count = int(rel.sum())
        rs = e.ReadStates(ps, count)
        msgs = SimpleNamespace(read_released=rel, term_commit=None, term_commit_index=None)
        stats = e.stats_buffer(dev)
        e.read_states(ps, book, rs, msgs=msgs, stats=stats)
        sd = e.stats_dict(e.stats_reduce(stats))
        assert int(rs.count.item()) == count == sd["vote_won"] + sd["vote_pending"], (count, sd)
        lib = e._lib.lib()

        # the structs built once: the timed window holds one ctypes call each,
        # the three launches of qe_read_states against the three of qe_collect
        p_s, b_s, o_s = ps.struct(), book.struct(), rs.struct()
        i_s = e._lib.QeReadStatesIn(read_released=e._ptr(rel))
        refs = (C.byref(p_s), C.byref(b_s), C.byref(i_s), C.byref(o_s))
        rs_scratch, stream = e._ptr(rs.scratch), e._stream(ps.device)

        def call():
            e._lib.check("qe_read_states", lib.qe_read_states(*refs, rs_scratch, None, stream))

        def collect():
            e._lib.check("qe_collect", lib.qe_collect(
                G, 0, None, e._ptr(rel), e._ptr(ps.committed), e._ptr(rs.group), e._ptr(rs.index),
                e._ptr(rs.count), e._ptr(scratch), e._stream(ps.device)))

        for _ in range(a.warmup):
            call()
            collect()
        torch.cuda.synchronize()
        t_rs, t_co = [], []
        for _ in range(a.runs):  # interleaved
            t_rs.append(event_ms(call))
            t_co.append(event_ms(collect))
        nbytes = algorithmic_bytes(G, count)
        d = {"records": count, "algorithmic_bytes": nbytes, "qe_read_states": summary(t_rs),
             "qe_collect": summary(t_co)}
        d["ratio"] = d["qe_read_states"]["median_ms"] / d["qe_collect"]["median_ms"]
        d["achieved_GBs"] = nbytes / (d["qe_read_states"]["median_ms"] * 1e-3) / 1e9
        d["hbm_frac"] = d["achieved_GBs"] / HBM_PEAK_GBS
        res["densities"][name] = d
        del rs
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
