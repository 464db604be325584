#!/usr/bin/env python3
"""qe_outbox on the state shape of the `propose` workload (16M groups, S = 5,
log_runs 4), at two densities: every group bcasts to its 4 followers, and one
group in 64 does.

Per density: the median time of qe_outbox (device events around the call, 20
runs after warm-up), the algorithmic bytes (every input the rule
must read, once, plus every record field written, once -- computed here from the
masks) and the fraction of the HBM peak they amount to.  qe_collect and
qe_heartbeat are timed in the same run as siblings.

The one comparison, against what a host did before: the device-to-host copy,
into pinned memory, of the rows duty H7 needs (sent, snap, msg_index, next,
peer, committed, last_index, run_first, run_term, run_count, term), against
qe_outbox plus the copy of min(count, capacity) records (count read first).
Host clock around work that ends in a synchronise; medians of 20.

  python scripts/outbox_bench.py [--groups N] [--runs K] [--out FILE]

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
S, R, E = 5, 4, 4


def algorithmic_bytes(G, groups, app, snap, hb, by_next=True, masks=2):
    """Per group the masks given (1 B each at S <= 8).  Per group with a
    message: term 8; with a MsgApp or a MsgSnap whose term comes from the runs,
    last_index 8 + run_count 1 + 16 * log_runs, and committed 8 with a MsgApp;
    snap_index 8 per group with a MsgSnap.  Per record: 46 written (group 8, to
    1, type 1, term 8, index 8, log_term 8, commit 8, ctx 4) + 12 * msg_runs;
    read: a MsgApp's index 8 (or the peer word 4 + Next 8), a heartbeat's
    commit 8.  (The upper bound of the per-group part: every group with a message
    is taken to have a MsgApp, which holds at both densities here.)"""
    per_group = 8 + 8 + 1 + 16 * R + 8
    rec = 46 + 12 * E
    return (G * masks + groups * per_group + snap * 8 + (app + snap + hb) * rec +
            app * (12 if by_next else 8) + hb * 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=1 << 24)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("outbox_bench: no GPU (there is no CPU fallback to time)")
    from etcd_amd import engine as e

    dev, G = "cuda:0", a.groups
    i64 = torch.int64
    ps = e.ProgressState(G, S, 4, R, dev, extras=("self_slot", "snap_index"))
    st = ps.stride
    g = torch.arange(G, device=dev, dtype=i64)
    r0 = 1000 + g % 7
    firsts = (r0, r0 + 5, r0 + 9)
    for r, (f, t) in enumerate(zip(firsts, (2, 3, 5))):
        ps.run_first[r * st:r * st + G] = f
        ps.run_term[r * st:r * st + G] = t
    ps.run_count.fill_(3)
    last = r0 + 12 + g % 5
    ps.last_index.copy_(last)
    ps.first_index.copy_(r0 + 1)
    ps.snap_index.copy_(r0)
    ps.committed.copy_(r0 + 9)
    ps.self_slot.copy_((g % S).to(torch.uint8))
    nxt0 = torch.ones(S * st, dtype=i64, device=dev)
    for s in range(S):
        lag = (g + s) % 6
        ps.next[s * st:s * st + G] = last - lag + 1   # after the call: all sent
        nxt0[s * st:s * st + G] = last - lag - 1      # before it: Index = Next - 1 is in the log
        ps.peer[s * st:s * st + G] = ((g + s) % 8 != 0).to(torch.int32)  # 1 = StateReplicate
        ps.match[s * st:s * st + G] = last - lag - 2
    term = torch.full((G,), 5, dtype=i64, device=dev)
    bcast = (0x1F ^ torch.bitwise_left_shift(torch.ones_like(g), g % S)).to(torch.uint8)
    gen = torch.Generator(device=dev).manual_seed(7)
    one_in_64 = torch.rand(G, device=dev, generator=gen) < 1.0 / 64
    snap = torch.zeros(G, dtype=torch.uint8, device=dev)
    msg_index = torch.zeros(S * st, dtype=i64, device=dev)

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

    res = {"groups": G, "slots": S, "log_runs": R, "msg_runs": E, "runs": a.runs,
           "hbm_peak_GBs": HBM_PEAK_GBS, "densities": {}}
    for name, sent in (("every_group", bcast),
                       ("one_in_64", torch.where(one_in_64, bcast, torch.zeros_like(bcast)))):
        groups = int((sent != 0).sum())
        count = 4 * groups
        ob = e.Outbox(ps, count, E)
        stats = e.stats_buffer(dev)
        e.outbox(ps, term, ob, sent=sent, snap=snap, next_before=nxt0, stats=stats)
        sd = e.stats_dict(e.stats_reduce(stats))
        assert int(ob.count.item()) == count == sd["vote_won"], (count, sd)  # all MsgApp, none BAD
        nbytes = algorithmic_bytes(G, groups, count, 0, 0)
        t = summary(dev_time(lambda: e.outbox(ps, term, ob, sent=sent, snap=snap,
                                              next_before=nxt0)))
        gbs = nbytes / (t["median_ms"] * 1e-3) / 1e9
        d = {"groups_with_message": groups, "records": count, "entries_listed": sd["commit_sum"],
             "algorithmic_bytes": nbytes, "qe_outbox": t, "achieved_GBs": gbs,
             "hbm_frac": gbs / HBM_PEAK_GBS}
        # the siblings, in the same run
        flags = (sent != 0).to(torch.uint8)
        scratch = torch.empty((e._lib.lib().qe_collect_scratch_bytes(G) + 7) // 8, dtype=i64,
                              device=dev)
        d["qe_collect"] = summary(dev_time(lambda: e._lib.check("qe_collect", e._lib.lib().qe_collect(
            G, 0, None, e._ptr(flags), e._ptr(ps.committed), e._ptr(ob.group), e._ptr(ob.index),
            e._ptr(ob.count), e._ptr(scratch), e._stream(ps.device)))))
        hb = e.heartbeat(ps)
        d["qe_heartbeat"] = summary(dev_time(lambda: e.heartbeat(ps, *hb)))
        # the comparison: the rows H7 walks, against the call and its list
        rows = [sent, snap, msg_index, ps.next, ps.peer, ps.committed, ps.last_index, ps.run_first,
                ps.run_term, ps.run_count, term]
        pinned = [torch.empty(r.shape, dtype=r.dtype, pin_memory=True) for r in rows]

        def copy_rows():
            for r, h in zip(rows, pinned):
                h.copy_(r, non_blocking=True)

        recs = [getattr(ob, k) for k in ("group", "to", "type", "term", "index", "log_term",
                                         "commit", "ctx")]
        ent = [ob.ent_len.view(E, -1), ob.ent_term.view(E, -1)]
        pin_recs = [torch.empty(r.shape, dtype=r.dtype, pin_memory=True) for r in recs + ent]

        def outbox_and_list():
            e.outbox(ps, term, ob, sent=sent, snap=snap, next_before=nxt0)
            n = min(int(ob.count.item()), ob.capacity)
            for r, h in zip(recs, pin_recs):
                h[:n].copy_(r[:n], non_blocking=True)
            for r, h in zip(ent, pin_recs[len(recs):]):
                h[:, :n].copy_(r[:, :n], non_blocking=True)

        d["host_rows_bytes"] = sum(r.numel() * r.element_size() for r in rows)
        d["list_bytes"] = count * (46 + 12 * E)
        d["copy_rows_h7"] = summary(wall_time(copy_rows))
        d["outbox_plus_list_copy"] = summary(wall_time(outbox_and_list))
        d["list_is_smaller"] = (d["outbox_plus_list_copy"]["median_ms"] <
                                d["copy_rows_h7"]["median_ms"])
        res["densities"][name] = d
        del ob, pinned, pin_recs
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
