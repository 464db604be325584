#!/usr/bin/env python3
"""qe_replies on 16M groups at S = 5, at two densities: every group answers a
MsgApp (QE_FR_APP_ACCEPT), and one group in 64 does.

Per density: the median time of qe_replies (device events around the call, 20
runs after warm-up), the algorithmic bytes (every input the rule
must read, once, plus every record field written, once -- computed here from the
result row) and the fraction of the HBM peak they amount to.  qe_collect and
qe_heartbeat are timed in the same run as siblings.

The one comparison, against what a host did before: the device-to-host copy,
into pinned memory, of the rows duty H8 needs (f_result, f_from, resp_index,
reject_hint, resp_log_term, term), against qe_replies plus the copy of
min(count, capacity) records (count read first).  Host clock around work that
ends in a synchronise; medians of 20.

  python scripts/replies_bench.py [--groups N] [--runs K] [--out FILE]

Prints one JSON document; --out also writes it to a file."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # the MI355X spec sheet: 8.0 TB/s
S = 5
RECORD_BYTES = 47      # group 8, to 1, type 1, term 8, index 8, log_term 8, hint 8, ctx 4, flags 1


def algorithmic_bytes(G, accepts, rejects=0, heartbeats=0, result_rows=1):
    """Per group 1 B per result row given.  Per answered group: from 1 + term 8
    + the kind's rows (an accept's resp_index 8; a reject's resp_index,
    reject_hint and resp_log_term 24; a heartbeat's context 4).  Per record 47
    written."""
    answered = accepts + rejects + heartbeats
    return (G * result_rows + answered * (1 + 8) + accepts * 8 + rejects * 24 + heartbeats * 4 +
            answered * RECORD_BYTES)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=1 << 24)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("replies_bench: no GPU (there is no CPU fallback to time)")
    from etcd_amd import engine as e

    dev, G = "cuda:0", a.groups
    i64, u8 = torch.int64, torch.uint8
    ps = e.ProgressState(G, S, 4, 4, dev, extras=("self_slot",))
    st = ps.stride
    g = torch.arange(G, device=dev, dtype=i64)
    last = 1012 + g % 5
    ps.last_index.copy_(last)
    ps.committed.copy_(1009 + g % 3)
    ps.self_slot.copy_((g % S).to(u8))
    for s in range(S):
        ps.match[s * st:s * st + G] = last - (g + s) % 6
    term = torch.full((G,), 5, dtype=i64, device=dev)
    lm = e.LeaderMsgs(ps, 0)
    lm.from_.copy_(((g + 1) % S).to(u8))
    fout = e.FollowerOut(ps)
    fout.resp_index.copy_(last)
    gen = torch.Generator(device=dev).manual_seed(7)
    one_in_64 = torch.rand(G, device=dev, generator=gen) < 1.0 / 64
    accept = torch.full((G,), e._lib.QE_FR_APP_ACCEPT, dtype=u8, device=dev)

    def dev_time(f):
        for _ in range(a.warmup):
            f()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.runs):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            f()
            t1.record()
            t1.synchronize()
            ts.append(t0.elapsed_time(t1))
        return ts

    def wall_time(f):
        for _ in range(a.warmup):
            f()
        ts = []
        for _ in range(a.runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts

    def summary(ts):
        return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}

    res = {"groups": G, "slots": S, "runs": a.runs, "hbm_peak_GBs": HBM_PEAK_GBS,
           "record_bytes": RECORD_BYTES, "densities": {}}
    for name, result in (("every_group", accept),
                         ("one_in_64", torch.where(one_in_64, accept, torch.zeros_like(accept)))):
        fout.result.copy_(result)
        count = int((result != 0).sum())
        rp = e.Replies(ps, count)
        stats = e.stats_buffer(dev)
        e.replies(ps, term, rp, follow=(lm, fout), stats=stats)
        sd = e.stats_dict(e.stats_reduce(stats))
        assert int(rp.count.item()) == count == sd["vote_won"], (count, sd)  # all MsgAppResp, none BAD
        nbytes = algorithmic_bytes(G, count)
        t = summary(dev_time(lambda: e.replies(ps, term, rp, follow=(lm, fout))))
        gbs = nbytes / (t["median_ms"] * 1e-3) / 1e9
        d = {"groups_answering": count, "records": count, "algorithmic_bytes": nbytes,
             "qe_replies": t, "achieved_GBs": gbs, "hbm_frac": gbs / HBM_PEAK_GBS}
        # the siblings, in the same run
        flags = (result != 0).to(u8)
        scratch = torch.empty((e._lib.lib().qe_collect_scratch_bytes(G) + 7) // 8, dtype=i64,
                              device=dev)
        d["qe_collect"] = summary(dev_time(lambda: e._lib.check("qe_collect", e._lib.lib().qe_collect(
            G, 0, None, e._ptr(flags), e._ptr(ps.committed), e._ptr(rp.group), e._ptr(rp.index),
            e._ptr(rp.count), e._ptr(scratch), e._stream(ps.device)))))
        hb = e.heartbeat(ps)
        d["qe_heartbeat"] = summary(dev_time(lambda: e.heartbeat(ps, *hb)))
        # the comparison: the rows H8 walks, against the call and its list
        rows = [fout.result, lm.from_, fout.resp_index, fout.reject_hint, fout.resp_log_term, term]
        pinned = [torch.empty(r.shape, dtype=r.dtype, pin_memory=True) for r in rows]

        def copy_rows():
            for r, h in zip(rows, pinned):
                h.copy_(r, non_blocking=True)

        recs = [getattr(rp, k) for k in ("group", "to", "type", "term", "index", "log_term",
                                         "hint", "ctx", "flags")]
        pin_recs = [torch.empty(r.shape, dtype=r.dtype, pin_memory=True) for r in recs]

        def replies_and_list():
            e.replies(ps, term, rp, follow=(lm, fout))
            n = min(int(rp.count.item()), rp.capacity)
            for r, h in zip(recs, pin_recs):
                h[:n].copy_(r[:n], non_blocking=True)

        d["host_rows_bytes"] = sum(r.numel() * r.element_size() for r in rows)
        d["list_bytes"] = count * RECORD_BYTES
        d["copy_rows_h8"] = summary(wall_time(copy_rows))
        d["replies_plus_list_copy"] = summary(wall_time(replies_and_list))
        d["list_is_faster"] = (d["replies_plus_list_copy"]["median_ms"] <
                               d["copy_rows_h8"]["median_ms"])
        res["densities"][name] = d
        del rp, pinned, pin_recs
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
