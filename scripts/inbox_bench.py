#!/usr/bin/env python3
"""qe_inbox on the shape of the `propose` workload (16M groups, S = 5, msg_runs
4), at two densities: about one delivered record per group, and one per 64
groups.  Even groups lead and receive MsgAppResp / MsgHeartbeatResp, odd groups
follow and receive MsgApp (with entry runs), MsgHeartbeat and MsgVote; the
receivers are drawn at random, so at the high density a third of the records
meets an occupied group and is deferred.

Per density: the median device time of qe_inbox (device events around the call,
20 runs after warm-up), the algorithmic bytes (every byte a pass must touch,
once per pass that needs it -- computed here from the list and the
dispositions) and the fraction of the HBM peak they amount to.  Siblings in the
same run, together the floor of the design: qe_collect over n flags, and a plain
fill of G * (3 + S) 32-bit words (the scratch the init pass resets).

The one comparison, against what a host does without the call: building the
four row families on the host from the same list -- WITH the dispositions given
for free, so the host only scatters (numpy) -- and uploading them from pinned
memory, and the bare upload of those rows with nothing built (the floor of any
host path), against uploading the list from pinned memory plus qe_inbox.  Host
clock around work that ends in a synchronise.

  python scripts/inbox_bench.py [--groups N] [--runs K] [--out FILE]

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
S, E = 5, 4
APP, HEARTBEAT, APP_RESP, HEARTBEAT_RESP, VOTE = 1, 3, 4, 6, 11
ROUTED, DEFERRED = 1, 3


def algorithmic_bytes(G, n, cnt):
    """cnt: records by kind.  The init pass writes (3 + S) scratch words and
    (3 + S) type bytes per group.  Every pass reads a record's group, from and
    type (10 B).  Pass 1: a 4-B atomic on first, one more on the cell of a
    response.  Pass 2: first (4) per record; cell (4), the message term (8) and
    the receiver's term (8) per response; a 4-B atomic per record that ends a
    wave.  Pass 3: first and stop (8), the disposition and the flag written (2);
    per response hi (4), the receiver's term and state (9); per wave member the
    message term (8); per routed record index and log_term (16) and its row: a
    MsgApp 8 + 48 read and 1 + 1 + 32 + 48 written, a MsgHeartbeat 8 read and 34
    written, a vote 1 read and 27 written, a response 8 + 4 read and 25 written.
    The deferred list: the flags twice (count, scatter) and 4 B per deferred."""
    init = G * 5 * (3 + S)
    keys = 3 * 10 * n
    p1 = 4 * n + 4 * cnt["resp"]
    p2 = 4 * n + 20 * cnt["resp"] + 4 * cnt["deferred"]
    p3 = 10 * n + 13 * cnt["resp"] + 8 * cnt["members"] + 16 * cnt["routed"]
    rows = (cnt["r_app"] * (56 + 82) + cnt["r_hb"] * (8 + 34) + cnt["r_vote"] * (1 + 27) +
            cnt["r_resp"] * (12 + 25))
    tail = 2 * n + 4 * cnt["deferred"]
    return init + keys + p1 + p2 + p3 + rows + tail


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=1 << 24)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    if not torch.cuda.is_available():
        sys.exit("inbox_bench: no GPU (there is no CPU fallback to time)")
    from etcd_amd import engine as e

    dev, G = "cuda:0", a.groups
    i64 = torch.int64
    ps = e.ProgressState(G, S, 4, 4, dev)
    st = ps.stride
    fol = e.Follower(ps)
    fol.term.fill_(5)
    g = torch.arange(G, device=dev, dtype=i64)
    fol.state.copy_(((g % 2 == 0) * 2).to(torch.uint8))  # even groups lead
    lm, sm, vm, pm = e.LeaderMsgs(ps, E), e.SnapMsgs(ps), e.VoteMsgs(ps), e.PeerMsgs(ps, False)

    def dev_time(f, runs=a.runs):
        for _ in range(a.warmup):
            f()
        torch.cuda.synchronize()
        ts = []
        for _ in range(runs):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            f()
            t1.record()
            t1.synchronize()
            ts.append(t0.elapsed_time(t1))
        return ts

    def wall_time(f, runs):
        f()
        ts = []
        for _ in range(runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts

    def summary(ts):
        return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}

    res = {"groups": G, "slots": S, "msg_runs": E, "runs": a.runs, "host_runs": a.host_runs,
           "hbm_peak_GBs": HBM_PEAK_GBS, "densities": {}}
    fill = torch.empty(G * (3 + S), dtype=torch.int32, device=dev)
    res["fill_scratch_words"] = summary(dev_time(lambda: fill.fill_(-1)))
    del fill
    rng = np.random.default_rng(7)
    for name, n in (("one_per_group", G), ("one_per_64_groups", G // 64)):
        grp = rng.integers(0, G, n).astype(np.uint64)
        kind = rng.random(n)
        lead = grp % 2 == 0
        typ = np.where(lead, np.where(kind < 0.8, APP_RESP, HEARTBEAT_RESP),
                       np.where(kind < 0.6, APP, np.where(kind < 0.9, HEARTBEAT, VOTE)))
        rec = dict(group=grp, type=typ.astype(np.uint8),
                   term=np.full(n, 5, np.uint64), index=grp + 100, log_term=np.full(n, 4, np.uint64),
                   commit=grp + 90, hint=np.zeros(n, np.uint64),
                   ent_len=np.tile(np.array([[3], [2], [0], [0]], np.uint32), (1, n)),
                   ent_term=np.tile(np.array([[4], [5], [0], [0]], np.uint64), (1, n)))
        rec["from"] = rng.integers(0, S, n).astype(np.uint8)
        ib = e.Inbox(ps, n, E, ctx=False, flags=False, src=False)
        ib.load_host(**rec)
        stats = e.stats_buffer(dev)
        e.inbox(ps, fol, ib, lm, sm, vm, pm, stats=stats)
        sd = e.stats_dict(e.stats_reduce(stats))
        disp, deferred = ib.results()
        routed = disp == ROUTED
        cnt = {"resp": int(lead.sum()), "deferred": int((disp == DEFERRED).sum()),
               "members": int((disp != DEFERRED).sum()), "routed": int(routed.sum()),
               "r_app": int((routed & (typ == APP)).sum()),
               "r_hb": int((routed & (typ == HEARTBEAT)).sum()),
               "r_vote": int((routed & (typ == VOTE)).sum()),
               "r_resp": int((routed & lead).sum())}
        assert cnt["deferred"] == len(deferred) and cnt["members"] == cnt["routed"], (cnt, sd)
        nbytes = algorithmic_bytes(G, n, cnt)
        t = summary(dev_time(lambda: e.inbox(ps, fol, ib, lm, sm, vm, pm)))
        gbs = nbytes / (t["median_ms"] * 1e-3) / 1e9
        d = {"records": n, "by_kind": cnt, "algorithmic_bytes": nbytes, "qe_inbox": t,
             "achieved_GBs": gbs, "hbm_frac": gbs / HBM_PEAK_GBS}
        L = e._lib.lib()
        flags = (ib.disposition[:n] == DEFERRED).to(torch.uint8)
        cs = torch.empty((L.qe_collect_scratch_bytes(n) + 7) // 8, dtype=i64, device=dev)
        cg, cc = torch.empty(n, dtype=i64, device=dev), torch.empty(1, dtype=i64, device=dev)
        d["qe_collect_n_flags"] = summary(dev_time(lambda: e._lib.check("qe_collect", L.qe_collect(
            n, 0, None, e._ptr(flags), None, e._ptr(cg), None, e._ptr(cc), e._ptr(cs),
            e._stream(dev)))))
        del flags, cs, cg
        # ---- the comparison: the list and the call, against rows built on the host ----
        fields = [getattr(ib, k)[:n] for k in ("group", "from_", "type", "term", "index",
                                               "log_term", "commit", "hint")]
        fields += [ib.ent_len[: E * n], ib.ent_term[: E * n]]
        pin_list = [torch.empty(f.shape, dtype=f.dtype, pin_memory=True) for f in fields]
        for f, h in zip(fields, pin_list):
            h.copy_(f)
        torch.cuda.synchronize()

        def list_and_inbox():
            for f, h in zip(fields, pin_list):
                f.copy_(h, non_blocking=True)
            e.inbox(ps, fol, ib, lm, sm, vm, pm)

        rows = [lm.type, lm.from_, lm.term, lm.index, lm.log_term, lm.commit, lm.ent_len,
                lm.ent_term, vm.type, vm.from_, vm.term, vm.index, vm.log_term, vm.flags,
                sm.type, sm.from_, sm.term, sm.snap_index, sm.snap_term,
                pm.type, pm.index, pm.reject_hint, pm.log_term]
        pin_rows = [torch.empty(r.shape, dtype=r.dtype, pin_memory=True) for r in rows]
        for h in pin_rows:
            h.zero_()
        hr = dict(zip(("f_type", "f_from", "f_term", "f_index", "f_log_term", "f_commit",
                       "f_ent_len", "f_ent_term", "v_type", "v_from", "v_term", "v_index",
                       "v_log_term", "v_flags", "s_type", "s_from", "s_term", "s_snap_index",
                       "s_snap_term", "r_type", "r_index", "r_hint", "r_log_term"),
                      [h.numpy() for h in pin_rows]))
        gi, fr = grp.astype(np.int64), rec["from"].astype(np.int64)
        sel_f = routed & ((typ == APP) | (typ == HEARTBEAT))
        sel_v, sel_r = routed & (typ == VOTE), routed & lead
        signed = {k: v.view(np.int64) if v.dtype == np.uint64 else v for k, v in rec.items()}

        def upload_rows():
            for r, h in zip(rows, pin_rows):
                r.copy_(h, non_blocking=True)

        def scatter_and_upload():
            for k in ("f_type", "v_type", "s_type", "r_type"):
                hr[k][:] = 0
            gf, gv, kr = gi[sel_f], gi[sel_v], fr[sel_r] * st + gi[sel_r]
            hr["f_type"][gf] = np.where(typ[sel_f] == APP, 1, 2)
            hr["f_from"][gf] = rec["from"][sel_f]
            for k in ("term", "index", "log_term", "commit"):
                hr["f_" + k][gf] = signed[k][sel_f]
            for j in range(E):
                hr["f_ent_len"][j * st + gf] = rec["ent_len"][j][sel_f].view(np.int32)
                hr["f_ent_term"][j * st + gf] = signed["ent_term"][j][sel_f]
            hr["v_type"][gv] = 1
            hr["v_from"][gv] = rec["from"][sel_v]
            for k in ("term", "index", "log_term"):
                hr["v_" + k][gv] = signed[k][sel_v]
            hr["r_type"][kr] = typ[sel_r] - 3
            hr["r_index"][kr] = signed["index"][sel_r]
            hr["r_hint"][kr] = signed["hint"][sel_r]
            hr["r_log_term"][kr] = signed["log_term"][sel_r]
            upload_rows()

        d["list_bytes"] = sum(f.numel() * f.element_size() for f in fields)
        d["host_rows_bytes"] = sum(r.numel() * r.element_size() for r in rows)
        d["upload_list_plus_qe_inbox"] = summary(wall_time(list_and_inbox, a.runs))
        d["upload_rows_nothing_built"] = summary(wall_time(upload_rows, a.runs))
        d["host_scatter_and_upload_rows"] = summary(wall_time(scatter_and_upload, a.host_runs))
        d["list_is_faster_than_bare_upload"] = (d["upload_list_plus_qe_inbox"]["median_ms"] <
                                                d["upload_rows_nothing_built"]["median_ms"])
        res["densities"][name] = d
        del ib, pin_list, pin_rows, hr, fields
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
