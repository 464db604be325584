#!/usr/bin/env python3
"""qe_tick against the kernels it fuses, at the heartbeat workload's shape
(16M groups x 5 slots, the leader in slot 0, a 0..4-entry ReadIndex queue).

  python scripts/tick_probe.py [--groups N] [--reps R] > profiles/tick_probe.txt

Variants, interleaved cycle by cycle in one process (a cycle = 10 calls =
one election timeout at ElectionTick 10 / HeartbeatTick 1), each call timed
with a device event pair:
  hb        qe_heartbeat alone
  hb+cq     qe_heartbeat every call, qe_check_quorum with the 10th
  tick(a)   every group a leader, CheckQuorum on: nine ticks beat, the tenth
            also checks the quorum (steady state: every follower was heard
            from since the last check, nobody steps down)
  tick(b)   every group a follower, no event, nobody past its timeout: the
            pure timer stream (7 B read, 5 B written per group)
  tick(c)   one leader in five, the others as (b)
Goal of (a): a beat-only tick takes no longer than qe_heartbeat's time scaled
by (heartbeat bytes + 12 timer bytes) / heartbeat bytes, with a 10 % margin.
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from etcd_amd import _lib, engine  # noqa: E402

ET, HT, S = 10, 1, 5
HB_BYTES = 1 + 8 + 1 + 4 + 4 + 1 + (S - 1) * 16  # bench.py's heartbeat bytes per group
TIMER_BYTES = 1 + 4 + 2 + 4 + 1                  # state, timer, timeout read; timer, action written
STREAM_CEILING = 6.29e12                          # profiles/r01_membw_ceiling.txt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=0, help="cycles per variant (0: >= 0.5 s each)")
    args = ap.parse_args()
    G, dev = args.groups, torch.device("cuda:0")
    lib = _lib.lib()
    ps = engine.ProgressState(G, S, 8, 1, dev, extras=("self_slot", "reads"))
    g = torch.arange(G, device=dev, dtype=torch.int64)
    h = ((g + 1) * 0x1E3779B97F4A7C15) >> 11  # (wraps: a cheap per-group hash)
    ps.last_index.copy_(1000 + (h & 0xFFFF))
    ps.committed.copy_(ps.last_index - 32)
    m = ps.match.view(S, ps.stride)
    for s in range(S):
        m[s, :G] = ps.last_index - ((h >> (4 * s + 16)) & 63) * (1 if s else 0)
    ps.self_slot.fill_(0)
    ps.read_count.copy_(((h >> 40) % 5).to(torch.uint8))
    ps.peer.fill_(_lib.QE_PR_REPLICATE | _lib.QE_PF_RECENT_ACTIVE)
    pristine = ps.peer.clone()
    p_ = ps.struct()
    stream = engine._stream(dev)
    commit = torch.zeros(S * ps.stride, dtype=torch.int64, device=dev)
    ctx = torch.zeros(G, dtype=torch.int32, device=dev)
    sent = torch.zeros(G, dtype=torch.uint8, device=dev)
    qa = torch.zeros(G, dtype=torch.uint8, device=dev)
    cp, xp, sp, qp = (engine._ptr(x) for x in (commit, ctx, sent, qa))

    def hb():
        engine.check("qe_heartbeat", lib.qe_heartbeat(C.byref(p_), cp, xp, sp, stream))

    def cq():
        engine.check("qe_check_quorum", lib.qe_check_quorum(C.byref(p_), qp, None, stream))

    def ticker(leader_every, beats):
        t = engine.Timers(G, ET, HT, True, 1, dev)
        if leader_every:
            t.state.copy_(torch.where(g % leader_every == 0, 2, 0).to(torch.uint8))
        t.randomized_timeout.fill_(60000 - 65536)  # no follower gets past its timeout
        out = engine.TickOut(ps, beats=beats)
        if not beats:
            out.hb_sent = None
        t_, o_ = t.struct(None, 1), out.struct()

        def call():
            engine.check("qe_tick", lib.qe_tick(C.byref(p_), C.byref(t_), C.byref(o_), None, stream))
        return call, t, out

    tick_a, ta, oa = ticker(1, True)
    tick_b, tb, ob = ticker(0, False)
    tick_c, tc, oc = ticker(5, True)
    variants = {"hb": [hb] * 10, "hb+cq": [hb] * 9 + [lambda: (hb(), cq())],
                "tick(a)": [tick_a] * 10, "tick(b)": [tick_b] * 10, "tick(c)": [tick_c] * 10}
    times = {k: [[] for _ in range(10)] for k in variants}

    def cycle(name, record):
        evs = []
        for i, f in enumerate(variants[name]):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            evs.append((a, b))
        ps.peer.copy_(pristine)  # the followers are heard from again (untimed)
        torch.cuda.synchronize(dev)
        if record:
            for i, (a, b) in enumerate(evs):
                times[name][i].append(a.elapsed_time(b))
        return sum(a.elapsed_time(b) for a, b in evs)

    for name in variants:  # warm-up: two cycles each
        cycle(name, False)
        per_cycle_ms = cycle(name, False)
    assert bool((oa.action == (_lib.QE_TICK_BEAT | _lib.QE_TICK_CHECKED_QUORUM)).all())
    assert bool((ta.state == 2).all()) and bool((ob.action == 0).all())
    reps = args.reps or max(20, int(500.0 / max(per_cycle_ms, 0.1)) + 1)
    for _ in range(reps):
        for name in variants:
            cycle(name, True)
    # a beat-only tick writes what qe_heartbeat writes
    hb()
    torch.cuda.synchronize(dev)
    c0, x0, s0 = commit.clone(), ctx.clone(), sent.clone()
    tick_a()
    torch.cuda.synchronize(dev)
    assert torch.equal(oa.hb_commit, c0) and torch.equal(oa.hb_ctx, x0) and torch.equal(oa.hb_sent, s0)

    def med(xs):
        xs = sorted(xs)
        return xs[len(xs) // 2]

    res = {"groups": G, "slots": S, "cycles_per_variant": reps}
    print(f"# qe_tick probe: {G} groups x {S} slots, ElectionTick {ET}, HeartbeatTick {HT}, "
          f"{reps} cycles of 10 calls per variant, interleaved; ms per call (median over cycles)")
    for name in variants:
        first9 = med([sum(times[name][i][r] for i in range(9)) / 9 for r in range(reps)])
        tenth = med(times[name][9])
        mean = med([sum(times[name][i][r] for i in range(10)) / 10 for r in range(reps)])
        res[name] = {"calls_1_9_ms": first9, "call_10_ms": tenth, "cycle_mean_ms": mean}
        print(f"{name:8s} calls 1-9 {first9:.4f}  call 10 {tenth:.4f}  cycle mean {mean:.4f}")
    t_hb = res["hb"]["calls_1_9_ms"]
    bw_hb = G * HB_BYTES / (t_hb * 1e-3)
    allowed = t_hb * (HB_BYTES + TIMER_BYTES) / HB_BYTES * 1.10
    beat = res["tick(a)"]["calls_1_9_ms"]
    print(f"(a) qe_heartbeat {t_hb:.4f} ms = {bw_hb / 1e12:.2f} TB/s over {HB_BYTES} B/group; a beat-only "
          f"tick {beat:.4f} ms; allowed {allowed:.4f} ms ({HB_BYTES + TIMER_BYTES} B/group at that "
          f"bandwidth + 10 %): {'met' if beat <= allowed else 'MISSED'}")
    print(f"(a) cycle mean: tick {res['tick(a)']['cycle_mean_ms']:.4f} ms against qe_heartbeat + "
          f"qe_check_quorum every 10th {res['hb+cq']['cycle_mean_ms']:.4f} ms")
    tb_ms = res["tick(b)"]["cycle_mean_ms"]
    bw_b = G * 12 / (tb_ms * 1e-3)
    print(f"(b) followers only: {tb_ms:.4f} ms = {bw_b / 1e12:.2f} TB/s over 12 B/group = "
          f"{100 * bw_b / STREAM_CEILING:.1f} % of the {STREAM_CEILING / 1e12:.2f} TB/s stream ceiling")
    print(f"(c) one leader in five: {res['tick(c)']['cycle_mean_ms']:.4f} ms per tick (cycle mean)")
    res["goal_a_allowed_ms"], res["goal_a_met"] = allowed, bool(beat <= allowed)
    res["b_share_of_stream_ceiling"] = bw_b / STREAM_CEILING
    print(json.dumps(res))


if __name__ == "__main__":
    main()
