#!/usr/bin/env python3
"""qe_follower_step at scale (16M groups, log_runs 4), next to qe_heartbeat
on the same state as the yardstick of the box.

  python scripts/follower_probe.py [--groups N] [--reps R] > profiles/follower_probe.txt

Launches, interleaved round by round in one process, each timed with a device
event pair; the state every launch starts from is restored (untimed) before
the next one:
  hb        qe_heartbeat (5 slots, the leader in slot 0)
  beat      a heartbeat-only launch (msg_runs 0): every group a follower at the
            message's term, the commit index advances
  steady    every group takes a one-run MsgApp of two entries at its tail, in
            the term of its last run: no run row and no run_count is written
  mixed     as steady, but one group in eight is rejected (LogTerm mismatch,
            the hint computed) or truncated (a higher-term leader overwrites
            its last three entries: a new run row)
Bytes per group are the algorithmic bytes of DESIGN.md §3's rules: every
field the reference logic needs, once, at field granularity.  The run rows
count as the kernel moves them: log_runs rows of 16 B for a group whose MsgApp
reaches the log.
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from etcd_amd import _lib, engine  # noqa: E402

S, R = 5, 4
HB_BYTES = 1 + 8 + 1 + 4 + 4 + 1 + (S - 1) * 16  # bench.py's heartbeat bytes per group
HBM_PEAK = 8.0e12
# read: type, from, m.Term, r.Term, state, m.Commit, committed, last_index
HEADER_RD = 1 + 1 + 8 + 8 + 1 + 8 + 8 + 8
APP_RD = 8 + 8 + 4 + 8          # m.Index, m.LogTerm, one entry run
RUNS_RD = 1 + R * 16            # run_count and the run rows
# written for every answered group: lead, result, events, resp_index, append_from
ANSWER_WR = 1 + 1 + 1 + 8 + 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=0, help="rounds (0: >= 0.5 s per launch kind)")
    args = ap.parse_args()
    G, dev = args.groups, torch.device("cuda:0")
    lib = _lib.lib()
    i64, u8 = torch.int64, torch.uint8
    ps = engine.ProgressState(G, S, 1, R, dev, extras=("self_slot", "reads"))
    g = torch.arange(G, device=dev, dtype=i64)
    h = ((g + 1) * 0x1E3779B97F4A7C15) >> 11  # (wraps: a cheap per-group hash)
    last = 1000 + (h & 0xFFFF)
    ps.last_index.copy_(last)
    ps.committed.copy_(last - 32)
    m = ps.match.view(S, ps.stride)
    for s in range(S):
        m[s, :G] = last - ((h >> (4 * s + 16)) & 63) * (1 if s else 0)
    ps.self_slot.fill_(0)
    ps.read_count.copy_(((h >> 40) % 5).to(u8))
    # the log: the dummy entry (0, 0), term 2 from index 1, term 3 over the last eight
    rf, rt = ps.run_first.view(R, ps.stride), ps.run_term.view(R, ps.stride)
    rf[1, :G], rt[1, :G] = 1, 2
    rf[2, :G], rt[2, :G] = last - 7, 3
    ps.run_count.fill_(3)
    fol = engine.Follower(ps)
    fol.term.fill_(3)
    fol.lead.fill_(1)
    state = {k: t.clone() for k, t in (("committed", ps.committed), ("last_index", ps.last_index),
                                       ("run_first", ps.run_first), ("run_term", ps.run_term),
                                       ("run_count", ps.run_count), ("term", fol.term),
                                       ("vote", fol.vote))}

    def restore():
        for k, t in state.items():
            (getattr(ps, k) if hasattr(ps, k) else getattr(fol, k)).copy_(t)

    p_, f_ = ps.struct(), fol.struct()
    stream = engine._stream(dev)
    out = engine.FollowerOut(ps)
    o_ = out.struct()

    def msgs(E, kind):
        lm = engine.LeaderMsgs(ps, E)
        lm.type.fill_(_lib.QE_LMSG_APP if E else _lib.QE_LMSG_HEARTBEAT)
        lm.from_.fill_(1)
        lm.term.fill_(3)
        lm.commit.copy_(last)
        if E:
            lm.index.copy_(last)
            lm.log_term.fill_(3)
            lm.ent_len[:G].fill_(2)
            lm.ent_term[:G].fill_(3)
        if kind == "mixed":
            rej, cut = (g % 16) == 3, (g % 16) == 11
            lm.log_term[rej] = 2
            lm.term[cut] = 4
            lm.index[cut] = last[cut] - 3
            lm.ent_len[:G][cut] = 3
            lm.ent_term[:G][cut] = 4
        return lm

    lms = {"beat": msgs(0, ""), "steady": msgs(1, ""), "mixed": msgs(1, "mixed")}
    structs = {k: v.struct() for k, v in lms.items()}
    commit = torch.zeros(S * ps.stride, dtype=i64, device=dev)
    ctx = torch.zeros(G, dtype=torch.int32, device=dev)
    sent = torch.zeros(G, dtype=u8, device=dev)
    cp, xp, sp = (engine._ptr(x) for x in (commit, ctx, sent))

    def hb():
        engine.check("qe_heartbeat", lib.qe_heartbeat(C.byref(p_), cp, xp, sp, stream))

    def follow(name):
        def call():
            engine.check("qe_follower_step",
                         lib.qe_follower_step(C.byref(p_), C.byref(f_), C.byref(structs[name]),
                                              C.byref(o_), None, stream))
        return call

    launches = {"hb": hb, "beat": follow("beat"), "steady": follow("steady"),
                "mixed": follow("mixed")}
    times = {k: [] for k in launches}

    def one(name, record):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launches[name]()
        b.record()
        torch.cuda.synchronize(dev)
        if record:
            times[name].append(a.elapsed_time(b))
        return a.elapsed_time(b)

    # what each launch did (checked once, on the warm-up), and its bytes
    FR = _lib
    want = {"beat": {FR.QE_FR_HEARTBEAT_RESP: G},
            "steady": {FR.QE_FR_APP_ACCEPT: G},
            "mixed": {FR.QE_FR_APP_REJECT: G // 16 + (G % 16 > 3),
                      FR.QE_FR_APP_ACCEPT: G - G // 16 - (G % 16 > 3)}}
    n_rej = want["mixed"][FR.QE_FR_APP_REJECT]
    n_cut = G // 16 + (G % 16 > 11)
    steady_b = HEADER_RD + APP_RD + RUNS_RD + ANSWER_WR + 8 + 8  # committed, last_index written
    bytes_per_group = {
        "hb": HB_BYTES,
        "beat": HEADER_RD + ANSWER_WR + 8,
        "steady": steady_b,
        # a rejection writes the hint and its term, not the log; a truncation also
        # writes term, vote, run_count and one run row
        "mixed": (steady_b * (G - n_rej - n_cut) + (steady_b - 16 + 16) * n_rej +
                  (steady_b + 8 + 1 + 1 + 16) * n_cut) / G,
    }
    slowest = 0.0
    for name in launches:
        for _ in range(2):
            restore()
            slowest = max(slowest, one(name, False))
        if name in want:
            got = torch.bincount(out.result.to(i64), minlength=32)
            assert {k: int(got[k]) for k in want[name]} == want[name], (name, got)
    assert bool((ps.run_count == torch.where((g % 16) == 11, 4, 3).to(u8)).all())
    reps = args.reps or max(20, int(500.0 / max(slowest, 0.1)) + 1)
    for _ in range(reps):
        for name in launches:
            restore()
            one(name, True)

    def med(xs):
        xs = sorted(xs)
        return xs[len(xs) // 2]

    res = {"groups": G, "log_runs": R, "rounds": reps}
    print(f"# qe_follower_step probe: {G} groups, log_runs {R}, {reps} rounds, launches interleaved; "
          f"median ms per launch, algorithmic bytes per group, share of the {HBM_PEAK / 1e12:.0f} TB/s HBM peak")
    for name in launches:
        t = med(times[name])
        bw = G * bytes_per_group[name] / (t * 1e-3)
        res[name] = {"ms": t, "bytes_per_group": bytes_per_group[name], "tb_per_s": bw / 1e12,
                     "share_of_hbm_peak": bw / HBM_PEAK, "min_ms": min(times[name]),
                     "max_ms": max(times[name])}
        print(f"{name:7s} {t:.4f} ms (min {min(times[name]):.4f}, max {max(times[name]):.4f})  "
              f"{bytes_per_group[name]:7.2f} B/group  {bw / 1e12:.2f} TB/s  "
              f"{100 * bw / HBM_PEAK:.1f} % of peak")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
