#!/usr/bin/env python3
"""qe_snapshot_step and qe_compact at scale (16M groups, 5 slots, log_runs 4),
next to qe_heartbeat and a heartbeat-only qe_follower_step on the same state
as the yardsticks of the box.

  python scripts/snapshot_probe.py [--groups N] [--reps R] > profiles/snapshot_probe.txt

Launches, interleaved round by round in one process, each timed with a device
event pair; the state every launch starts from is restored (untimed) before
the next one:
  hb        qe_heartbeat (5 slots, the leader in slot 0)
  beat      qe_follower_step, heartbeat-only (msg_runs 0)
  none      qe_snapshot_step, no group has a message
  sparse    qe_snapshot_step, one MsgSnap per 64-group tile, restored
  restore   qe_snapshot_step, every group restored (no cs_ids)
  compact0  qe_compact, every group compacted inside its first run (r* = 0:
            one run_first word moves)
  compact1  qe_compact, every group compacted inside its second run (r* = 1:
            the table moves down one row)
Bytes per group are the algorithmic bytes of DESIGN.md §3's rules: every
field the logic needs, once, at field granularity, the run rows as the kernels
move them.
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
BEAT_BYTES = 43 + 19 + 8                         # DESIGN.md §5, the follower's heartbeat
HBM_PEAK = 8.0e12
# qe_snapshot_step: type | from, m.Term, r.Term, state, snapshot index, committed
NONE_B = 1 + 2                                   # type read; result, events written
HEADER_RD = 1 + 1 + 8 + 8 + 1 + 8 + 8
# self_slot, four masks, auto_leave, snapshot term, last_index, run_count
RESTORE_RD = 1 + 4 + 1 + 8 + 8 + 1
# lead, result, events, resp_index, committed, last_index, run row 0, run_count,
# first_index, snap_index, six masks, auto_leave
RESTORE_WR = 1 + 1 + 1 + 8 + 8 + 8 + 16 + 1 + 8 + 8 + 6 + 1
RESTORE_B = HEADER_RD + RESTORE_RD + RESTORE_WR
# qe_compact: compact_index, committed, last_index, applied, run_count, run_first rows |
# run_first[0], first_index, result
COMPACT0_B = 8 + 8 + 8 + 8 + 1 + R * 8 + 8 + 8 + 1
# + the run_term rows read, run_count, run_term[0] and one moved row written
COMPACT1_B = COMPACT0_B + R * 8 + 1 + 8 + 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=0, help="rounds (0: >= 0.5 s per launch kind)")
    args = ap.parse_args()
    G, dev = args.groups, torch.device("cuda:0")
    lib = _lib.lib()
    i64, u8 = torch.int64, torch.uint8
    ps = engine.ProgressState(G, S, 1, R, dev, extras=("self_slot", "reads", "snap_index"))
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
    # the log: the dummy entry (100, 1), term 2 from index 500, term 3 over the last eight
    rf, rt = ps.run_first.view(R, ps.stride), ps.run_term.view(R, ps.stride)
    rf[0, :G], rt[0, :G] = 100, 1
    rf[1, :G], rt[1, :G] = 500, 2
    rf[2, :G], rt[2, :G] = last - 7, 3
    ps.run_count.fill_(3)
    ps.first_index.fill_(101)
    ps.snap_index.fill_(100)
    fol = engine.Follower(ps)
    fol.term.fill_(3)
    fol.lead.fill_(1)
    conf = engine.ConfState(G, S, dev)
    conf.slot_ids = None
    names = ("committed", "last_index", "run_first", "run_term", "run_count", "first_index",
             "snap_index")
    state = {k: getattr(ps, k).clone() for k in names}
    state.update(term=fol.term.clone(), vote=fol.vote.clone(), lead=fol.lead.clone())

    def restore():
        for k, t in state.items():
            (getattr(ps, k) if k in names else getattr(fol, k)).copy_(t)

    p_, f_, c_ = ps.struct(), fol.struct(), conf.struct()
    stream = engine._stream(dev)
    fout, sout = engine.FollowerOut(ps), engine.SnapOut(ps)
    fo_, so_ = fout.struct(), sout.struct()
    beat = engine.LeaderMsgs(ps, 0)
    beat.type.fill_(_lib.QE_LMSG_HEARTBEAT)
    beat.from_.fill_(1)
    beat.term.fill_(3)
    beat.commit.copy_(last)
    beat_ = beat.struct()

    def snap_msgs(kind):
        sm = engine.SnapMsgs(ps)
        if kind == "restore":
            sm.type.fill_(_lib.QE_SMSG_SNAP)
        elif kind == "sparse":
            sm.type.copy_(((g % 64) == 17).to(u8))
        sm.from_.fill_(1)
        sm.term.fill_(3)
        sm.snap_index.copy_(last + 1000)
        sm.snap_term.fill_(3)
        sm.cs_inc.fill_((1 << S) - 1)
        return sm

    sms = {k: snap_msgs(k) for k in ("none", "sparse", "restore")}
    sm_ = {k: v.struct() for k, v in sms.items()}

    def compaction(ci):
        cp = engine.Compaction(ps, create=False)
        cp.compact_index.fill_(ci)
        cp.applied.copy_(last - 40)
        return cp

    cps = {"compact0": compaction(300), "compact1": compaction(700)}
    cp_ = {k: v.struct() for k, v in cps.items()}
    commit = torch.zeros(S * ps.stride, dtype=i64, device=dev)
    ctx = torch.zeros(G, dtype=torch.int32, device=dev)
    sent = torch.zeros(G, dtype=u8, device=dev)
    cp, xp, sp = (engine._ptr(x) for x in (commit, ctx, sent))

    def hb():
        engine.check("qe_heartbeat", lib.qe_heartbeat(C.byref(p_), cp, xp, sp, stream))

    def follow():
        engine.check("qe_follower_step",
                     lib.qe_follower_step(C.byref(p_), C.byref(f_), C.byref(beat_), C.byref(fo_),
                                          None, stream))

    def snap(name):
        def call():
            engine.check("qe_snapshot_step",
                         lib.qe_snapshot_step(C.byref(p_), C.byref(f_), C.byref(c_),
                                              C.byref(sm_[name]), C.byref(so_), None, stream))
        return call

    def compact(name):
        def call():
            engine.check("qe_compact", lib.qe_compact(C.byref(p_), C.byref(cp_[name]), None, stream))
        return call

    launches = {"hb": hb, "beat": follow, "none": snap("none"), "sparse": snap("sparse"),
                "restore": snap("restore"), "compact0": compact("compact0"),
                "compact1": compact("compact1")}
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

    n_sparse = G // 64 + (G % 64 > 17)
    bytes_per_group = {
        "hb": HB_BYTES, "beat": BEAT_BYTES, "none": NONE_B,
        "sparse": (NONE_B * (G - n_sparse) + RESTORE_B * n_sparse) / G,
        "restore": RESTORE_B, "compact0": COMPACT0_B, "compact1": COMPACT1_B,
    }
    # what each launch did (checked once, on the warm-up)
    want = {"none": {_lib.QE_SR_NONE: G}, "sparse": {_lib.QE_SR_RESTORED: n_sparse},
            "restore": {_lib.QE_SR_RESTORED: G}, "compact0": {_lib.QE_CP_COMPACTED: G},
            "compact1": {_lib.QE_CP_COMPACTED: G}}
    want_count = {"compact0": 3, "compact1": 2, "restore": 1}
    slowest = 0.0
    for name in launches:
        for _ in range(2):
            restore()
            slowest = max(slowest, one(name, False))
        if name in want:
            res = cps[name].result if name in cps else sout.result
            got = torch.bincount(res.to(i64), minlength=32)
            assert {k: int(got[k]) for k in want[name]} == want[name], (name, got)
        if name in want_count:
            assert bool((ps.run_count == want_count[name]).all()), name
    reps = args.reps or max(20, int(500.0 / max(slowest, 0.1)) + 1)
    for _ in range(reps):
        for name in launches:
            restore()
            one(name, True)

    def med(xs):
        xs = sorted(xs)
        return xs[len(xs) // 2]

    res = {"groups": G, "slots": S, "log_runs": R, "rounds": reps}
    print(f"# snapshot probe: {G} groups, {S} slots, log_runs {R}, {reps} rounds, launches "
          f"interleaved; median ms per launch, algorithmic bytes per group, share of the "
          f"{HBM_PEAK / 1e12:.0f} TB/s HBM peak")
    for name in launches:
        t = med(times[name])
        bw = G * bytes_per_group[name] / (t * 1e-3)
        res[name] = {"ms": t, "bytes_per_group": bytes_per_group[name], "tb_per_s": bw / 1e12,
                     "share_of_hbm_peak": bw / HBM_PEAK, "min_ms": min(times[name]),
                     "max_ms": max(times[name])}
        print(f"{name:8s} {t:.4f} ms (min {min(times[name]):.4f}, max {max(times[name]):.4f})  "
              f"{bytes_per_group[name]:7.2f} B/group  {bw / 1e12:.2f} TB/s  "
              f"{100 * bw / HBM_PEAK:.1f} % of peak")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
