#!/usr/bin/env python3
"""Time qe_ready, and qe_advance on the lists it produced, on the device.

    python scripts/ready_bench.py [--groups 16777216] [--repeats 20] [--warmup 3]

G groups x S = 5 slots, one term run, ent_runs 4, at three densities of listed
groups: 1 in 64, 1 in 4, all.  A listed group has two entries to persist, one
to apply and a HardState delta (MustSync); every other group is quiet.  The
floor beside it, in the same process and on the same groups: qe_collect over
a flag row with the same groups flagged, values gathered.  Times are device
events around each call, after a warm-up, the calls of a repeat interleaved
(ready, collect, advance, then the next density); the median and the spread of
the repeats are printed, and one JSON line at the end.

Bytes are the algorithm's, computed here from the shape: the count pass reads
9 u64 rows and 6 or 7 byte rows of every group and writes its flag byte; the
fill reads the flag byte of every group and, for a listed group, its rows once
more with run_count and the run table, and writes the record.  The fraction of
peak is those bytes over the measured time over the HBM peak given on the
command line (default 8 TB/s, the MI355X's)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from etcd_amd import engine as e  # noqa: E402

S, F, R, E = 5, 1, 1, 4
COUNT_READ = 9 * 8 + 6 + 1          # the u64 rows, the byte rows with vote, the flag written
FILL_LISTED = 8 * 8 + 6 + 1 + 2 * 8 * R   # its rows again, run_count, the run table
RECORD = 9 * 8 + 4 + 2 * E * (4 + 8)     # the record written


def build(G, every, dev):
    ps = e.ProgressState(G, S, F, R, dev)
    fol = e.Follower(ps)
    ps.run_count.fill_(1)
    ps.run_term[:G].fill_(1)
    ps.last_index.fill_(10)
    ps.committed.fill_(8)
    fol.term.fill_(1)
    fol.vote.fill_(0)
    fol.lead.fill_(0)
    rs = e.ReadyState(ps).reset(ps, fol)
    rs.applied.copy_(ps.committed)
    listed = torch.zeros(G, dtype=torch.uint8, device=dev)
    listed[::every] = 1
    on = listed.bool()
    ps.last_index[on] += 2
    ps.committed[on] += 1
    fol.term[on] += 1
    return ps, fol, rs, listed


def case(G, every, dev):
    ps, fol, rs, listed = build(G, every, dev)
    n = (G + every - 1) // every
    rd = e.Ready(ps, n, E)
    keep = {k: getattr(rs, k).clone() for k in rs.ARRAYS}
    out_g = torch.zeros(n, dtype=torch.int64, device=dev)
    out_v = torch.zeros(n, dtype=torch.int64, device=dev)
    scratch = torch.empty((e._lib.lib().qe_collect_scratch_bytes(G) + 7) // 8 + 1,
                          dtype=torch.int64, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)

    def collect():
        e.check("qe_collect", e._lib.lib().qe_collect(
            G, 0, None, e._ptr(listed), e._ptr(ps.committed), e._ptr(out_g), e._ptr(out_v),
            e._ptr(cnt), e._ptr(scratch), e._stream(ps.device)))

    def restore():
        for k, t in keep.items():
            getattr(rs, k).copy_(t)

    return dict(ps=ps, fol=fol, rs=rs, rd=rd, n=n, collect=collect, restore=restore,
                t={"ready": [], "collect": [], "advance": []})


def timed(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=1 << 24)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--peak-tbs", type=float, default=8.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ready_bench: no GPU (this measurement has no CPU form)")
    dev, G = "cuda:0", a.groups
    cases = {every: case(G, every, dev) for every in (64, 4, 1)}
    for rep in range(a.warmup + a.repeats):
        for every, c in cases.items():
            t_r = timed(lambda: e.ready(c["ps"], c["fol"], c["rs"], c["rd"]))
            t_c = timed(c["collect"])
            t_a = timed(lambda: e.advance(c["ps"], c["rs"], c["rd"]))
            if rep == 0:
                assert int(c["rd"].count.item()) == c["n"], (every, int(c["rd"].count.item()))
                res = c["rd"].result[:c["n"]]
                assert bool((res == e._lib.QE_ADV_OK).all())
                e.ready(c["ps"], c["fol"], c["rs"], c["rd"])
                assert int(c["rd"].count.item()) == 0  # everything advanced
            c["restore"]()
            if rep >= a.warmup:
                for k, v in (("ready", t_r), ("collect", t_c), ("advance", t_a)):
                    c["t"][k].append(v)
    out = {"groups": G, "slots": S, "ent_runs": E, "repeats": a.repeats, "cases": []}
    for every, c in cases.items():
        n = c["n"]
        nbytes = G * (COUNT_READ + 1) + n * (FILL_LISTED + RECORD)
        row = {"listed_one_in": every, "records": n, "algorithmic_bytes": nbytes}
        for k, ts in c["t"].items():
            row[k + "_ms"] = round(statistics.median(ts), 4)
            row[k + "_ms_min_max"] = [round(min(ts), 4), round(max(ts), 4)]
        row["ready_fraction_of_hbm_peak"] = round(
            nbytes / (row["ready_ms"] * 1e-3) / (a.peak_tbs * 1e12), 3)
        out["cases"].append(row)
        print(f"1 in {every:2d}: {n:9d} records, qe_ready {row['ready_ms']:.3f} ms "
              f"{row['ready_ms_min_max']}, qe_collect {row['collect_ms']:.3f} ms, qe_advance "
              f"{row['advance_ms']:.3f} ms; {nbytes / G:.1f} B/group, "
              f"{row['ready_fraction_of_hbm_peak']:.1%} of {a.peak_tbs} TB/s")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
