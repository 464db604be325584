#!/usr/bin/env python3
"""qe_vote_step at scale (16M groups, 5 slots, log_runs 4), next to the
heartbeat-only qe_follower_step and qe_heartbeat on the same state as the
yardsticks of the box (the same idiom, similar bytes).

  python scripts/vote_probe.py [--groups N] [--reps R] > profiles/vote_probe.txt

Launches, interleaved round by round in one process, each timed with a device
event pair; the state every launch starts from is restored (untimed) before
the next one:
  hb        qe_heartbeat (the leader in slot 0)
  beat      qe_follower_step, heartbeat-only (msg_runs 0)
  grant     (a) a voter-only launch: every group a follower at term 3 with no
            leader and no vote takes a MsgVote of term 4 whose log is its own:
            becomeFollower(4), the vote granted
  mixed     (b) as (a) under CheckQuorum, but one group in eight is rejected
            (the candidate's last term is behind) and one in eight knows a
            leader and is in lease
  resp      (c) a full launch: every group a candidate of five voters that has
            its own vote takes a granting MsgVoteResp; half of them hold an
            earlier grant and win, the others stay pending
Bytes per group are the algorithmic bytes of DESIGN.md §3's rules: every field
the reference logic needs, once, at field granularity.
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from etcd_amd import _lib, engine  # noqa: E402

S, R, ET = 5, 4, 10
HB_BYTES = 1 + 8 + 1 + 4 + 4 + 1 + (S - 1) * 16  # bench.py's heartbeat bytes per group
BEAT_BYTES = (1 + 1 + 8 + 8 + 1 + 8 + 8 + 8) + (1 + 1 + 1 + 8 + 8) + 8  # scripts/follower_probe.py
HBM_PEAK = 8.0e12
# read for every message: type, from, m.Term, flags, r.Term, state, lead, vote
HEADER_RD = 1 + 1 + 8 + 1 + 8 + 1 + 1 + 1
REQ_RD = 8 + 8            # m.Index, m.LogTerm
LOG_RD = 8 + 1 + 8        # last_index, run_count, the last run's term
ALWAYS_WR = 1 + 1 + 1     # result, events, elected


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
    timer = torch.full((G,), 3, dtype=torch.int32, device=dev)  # electionElapsed 3 < ET
    voters = {"grant": engine.Voter(ps, votes=False, election_timeout=ET),
              "mixed": engine.Voter(ps, votes=False, check_quorum=True, election_timeout=ET),
              "resp": engine.Voter(ps, votes=True, election_timeout=ET)}
    voters["mixed"].timer = timer
    vr = voters["resp"]
    lease, behind, early = (g % 8) == 3, (g % 8) == 6, (g % 2) == 1

    # the state each launch kind starts from: (term, state, lead, vote, voted, granted)
    def start(name):
        term = torch.full((G,), 3, dtype=i64, device=dev)
        state = torch.zeros(G, dtype=u8, device=dev)
        lead = torch.full((G,), 0xFF, dtype=u8, device=dev)
        vote = torch.full((G,), 0xFF, dtype=u8, device=dev)
        voted = torch.zeros(G, dtype=u8, device=dev)
        if name == "beat":
            lead.fill_(1)
        if name == "mixed":
            lead[lease] = 2
        if name == "resp":
            term.fill_(4)
            state.fill_(_lib.QE_STATE_CANDIDATE)
            vote.fill_(0)
            voted.fill_(1)
            voted[early] = 1 | 4
        return {"term": term, "state": state, "lead": lead, "vote": vote, "voted": voted,
                "granted": voted.clone(), "committed": ps.committed.clone()}

    starts = {k: start(k) for k in ("hb", "beat", "grant", "mixed", "resp")}

    def restore(name):
        st = starts[name]
        for k in ("term", "state", "lead", "vote"):
            getattr(fol, k).copy_(st[k])
        vr.voted.copy_(st["voted"])
        vr.granted.copy_(st["granted"])
        ps.committed.copy_(st["committed"])

    p_, f_ = ps.struct(), fol.struct()
    stream = engine._stream(dev)
    out, fout = engine.VoteOut(ps), engine.FollowerOut(ps)
    o_, fo_ = out.struct(), fout.struct()

    def vmsgs(name):
        vm = engine.VoteMsgs(ps)
        vm.from_.fill_(1)
        vm.term.fill_(4)
        if name == "resp":
            vm.type.fill_(_lib.QE_VMSG_VOTE_RESP)
            return vm
        vm.type.fill_(_lib.QE_VMSG_VOTE)
        vm.index.copy_(last)
        vm.log_term.fill_(3)
        if name == "mixed":
            vm.log_term[behind] = 2
        return vm

    vms = {k: vmsgs(k) for k in voters}
    vstructs = {k: (voters[k].struct(), vms[k].struct()) for k in voters}
    lm = engine.LeaderMsgs(ps, 0)
    lm.type.fill_(_lib.QE_LMSG_HEARTBEAT)
    lm.from_.fill_(1)
    lm.term.fill_(3)
    lm.commit.copy_(last)
    lm_ = lm.struct()
    commit = torch.zeros(S * ps.stride, dtype=i64, device=dev)
    ctx = torch.zeros(G, dtype=torch.int32, device=dev)
    sent = torch.zeros(G, dtype=u8, device=dev)
    cp, xp, sp = (engine._ptr(x) for x in (commit, ctx, sent))

    def hb():
        engine.check("qe_heartbeat", lib.qe_heartbeat(C.byref(p_), cp, xp, sp, stream))

    def beat():
        engine.check("qe_follower_step",
                     lib.qe_follower_step(C.byref(p_), C.byref(f_), C.byref(lm_), C.byref(fo_),
                                          None, stream))

    def vote(name):
        v_, m_ = vstructs[name]

        def call():
            engine.check("qe_vote_step",
                         lib.qe_vote_step(C.byref(p_), C.byref(f_), C.byref(v_), C.byref(m_),
                                          C.byref(o_), None, stream))
        return call

    launches = {"hb": hb, "beat": beat, "grant": vote("grant"), "mixed": vote("mixed"),
                "resp": vote("resp")}
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
    n8 = lambda k: G // 8 + (G % 8 > k)  # noqa: E731  groups with g % 8 == k
    n_lease, n_behind, n_early = n8(3), n8(6), G // 2
    VR = _lib
    want = {"grant": {VR.QE_VR_GRANT: G},
            "mixed": {VR.QE_VR_GRANT: G - n_lease - n_behind, VR.QE_VR_REJECT: n_behind,
                      VR.QE_VR_IN_LEASE: n_lease},
            "resp": {VR.QE_VR_WON: n_early, VR.QE_VR_PENDING: G - n_early}}
    # a granted MsgVote of a higher term writes term, vote and resp_term (state
    # and lead hold follower / none already); a rejected one term and resp_term
    grant_b = HEADER_RD + REQ_RD + LOG_RD + ALWAYS_WR + 8 + 1 + 8
    # under CheckQuorum the timer (4 B); in lease nothing but the three output rows
    # is written and the log is not needed
    mixed_b = ((grant_b + 4) * (G - n_lease - n_behind) + (grant_b + 4 - 1) * n_behind +
               (HEADER_RD + 4 + ALWAYS_WR) * n_lease) / G
    # a response: self_slot, voted, granted read; pending writes the two masks, a
    # win state, lead and the two masks
    resp_rd = HEADER_RD + 1 + 1 + 1
    resp_b = ((resp_rd + ALWAYS_WR + 2) * (G - n_early) + (resp_rd + ALWAYS_WR + 4) * n_early) / G
    bytes_per_group = {"hb": HB_BYTES, "beat": BEAT_BYTES, "grant": grant_b, "mixed": mixed_b,
                       "resp": resp_b}
    slowest = 0.0
    for name in launches:
        for _ in range(2):
            restore(name)
            slowest = max(slowest, one(name, False))
        if name in want:
            got = torch.bincount(out.result.to(i64), minlength=32)
            assert {k: int(got[k]) for k in want[name]} == want[name], (name, got)
    reps = args.reps or max(20, int(500.0 / max(slowest, 0.1)) + 1)
    for _ in range(reps):
        for name in launches:
            restore(name)
            one(name, True)

    def med(xs):
        xs = sorted(xs)
        return xs[len(xs) // 2]

    res = {"groups": G, "log_runs": R, "rounds": reps}
    print(f"# qe_vote_step probe: {G} groups, {S} slots, log_runs {R}, {reps} rounds, launches "
          f"interleaved; median ms per launch, algorithmic bytes per group, share of the "
          f"{HBM_PEAK / 1e12:.0f} TB/s HBM peak")
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
