#!/usr/bin/env python3
"""qe_requests at 16M groups (S = 5) with n = G / 64 and n = G records, next to
qe_inbox at the same G, S and n in the same process.  Both lists are random:
uniform receivers, half of the groups leading, local terms; qe_requests gets
proposals, reads, transfers and read responses in equal parts, qe_inbox the
seven response types (its class R, the one that shares a wave).  Device events
around one C call with its structs built beforehand (the window holds the
host's enqueue of the launches); after warm-up the two calls are interleaved
call by call, medians of K runs with the minimum and the maximum.

qe_inbox is the yardstick: existing code, one more record pass and 3 + S
scratch words per group against one.

  python scripts/time_requests.py [--groups N] [--runs K] [--out FILE]

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

S = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=1 << 24)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("time_requests: no GPU (there is no CPU fallback to time)")
    from etcd_amd import _lib
    from etcd_amd import engine as e

    dev, G = "cuda:0", a.groups
    i64, u8 = torch.int64, torch.uint8
    lib = _lib.lib()
    gen = torch.Generator(device=dev).manual_seed(11)
    rnd = lambda hi, n: torch.randint(0, hi, (n,), device=dev, generator=gen)  # noqa: E731
    ps = e.ProgressState(G, S, 1, 1, dev, extras=("self_slot",))
    ps.self_slot.copy_((torch.arange(G, device=dev) % S).to(u8))
    fol = e.Follower(ps)
    fol.term.fill_(3)
    fol.state.copy_((rnd(2, G) * 2).to(u8))          # follower / leader
    fol.lead.copy_(rnd(S, G).to(u8))
    lm, sm, vm, pm = e.LeaderMsgs(ps, 0), e.SnapMsgs(ps), e.VoteMsgs(ps), e.PeerMsgs(ps, outputs=False)
    props = e.Proposals(ps)

    def event_ms(f):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        f()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1)

    def summary(ts):
        return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}

    res = {"groups": G, "slots": S, "runs": a.runs, "lists": {}}
    for name, n in (("G_over_64", G // 64), ("G", G)):
        group = rnd(G, n).to(i64)
        frm = rnd(S, n).to(u8)
        # ---- qe_requests ----
        rq = e.Requests(ps, n, src=False)
        rq.q_group.copy_(group)
        rq.q_from_.copy_(frm)
        rq.q_type.copy_(torch.tensor([10, 17, 18, 19], device=dev, dtype=u8)[rnd(4, n)])
        rq.q_num_entries.fill_(1)
        rq.q_key.copy_(torch.arange(n, device=dev, dtype=i64) * 7919 + 1)
        rq.n = n
        stats = e.stats_buffer(dev)
        e.requests(ps, fol, rq, props, pm, vm, stats=stats)
        sd = e.stats_reduce(stats).cpu().numpy()
        disp = {k: int(sd[getattr(_lib, "QE_STAT_REQ_" + k)]) for k in (
            "ROUTED", "DEFERRED", "FORWARDED", "READ_STATE", "NO_ARM", "BAD")}
        assert sum(disp.values()) == n and disp["BAD"] == 0, disp
        p_s, f_s = ps.struct(), fol.struct()
        qi = _lib.QeRequestsIn(
            n, 0, 0, e._ptr(rq.q_group), e._ptr(rq.q_type), e._ptr(rq.q_from_), e._ptr(rq.q_term),
            e._ptr(rq.q_index), e._ptr(rq.q_key), e._ptr(rq.q_num_entries), None, None, None, None,
            None, 0)
        qo = _lib.QeRequestsOut(
            e._ptr(props.num_entries), None, None, None, None, None, 0, e._ptr(rq.ri_request),
            e._ptr(rq.ri_key), e._ptr(rq.ri_from), e._ptr(vm.type), e._ptr(vm.from_),
            e._ptr(vm.term), e._ptr(vm.index), e._ptr(vm.log_term), e._ptr(vm.flags),
            e._ptr(pm.type), None, None, None, None, e._ptr(rq.disposition),
            e._ptr(rq.deferred_pos), e._ptr(rq.deferred_count), rq.capacity,
            *[e._ptr(getattr(rq, k)) for k in rq.ARRAYS])
        q_refs = (C.byref(p_s), C.byref(f_s), C.byref(qi), C.byref(qo))
        q_scratch, stream = e._ptr(rq.scratch), e._stream(ps.device)

        def requests():
            _lib.check("qe_requests", lib.qe_requests(*q_refs, q_scratch, None, stream))

        # ---- qe_inbox ----
        ib = e.Inbox(ps, n, 0, ctx=False, flags=False, src=False)
        ib.group.copy_(group)
        ib.from_.copy_(frm)
        ib.type.copy_((4 + rnd(7, n)).to(u8))
        ib.n = n
        e.inbox(ps, fol, ib, lm, sm, vm, pm)
        ii = _lib.QeInboxIn(n, 0, 0, e._ptr(ib.group), e._ptr(ib.from_), e._ptr(ib.type),
                            e._ptr(ib.term), e._ptr(ib.index), e._ptr(ib.log_term),
                            e._ptr(ib.commit), e._ptr(ib.hint), None, None, None, None, None)
        io = _lib.QeInboxOut(
            e._ptr(lm.type), e._ptr(lm.from_), e._ptr(lm.term), e._ptr(lm.index),
            e._ptr(lm.log_term), e._ptr(lm.commit), None, None, e._ptr(sm.type), e._ptr(sm.from_),
            e._ptr(sm.term), e._ptr(sm.snap_index), e._ptr(sm.snap_term), e._ptr(vm.type),
            e._ptr(vm.from_), e._ptr(vm.term), e._ptr(vm.index), e._ptr(vm.log_term),
            e._ptr(vm.flags), e._ptr(pm.type), e._ptr(pm.index), e._ptr(pm.reject_hint),
            e._ptr(pm.log_term), None, None, None, None, None, e._ptr(ib.disposition),
            e._ptr(ib.deferred), e._ptr(ib.deferred_count))
        i_refs = (C.byref(p_s), C.byref(f_s), C.byref(ii), C.byref(io))
        i_scratch = e._ptr(ib.scratch)

        def inbox():
            _lib.check("qe_inbox", lib.qe_inbox(*i_refs, i_scratch, None, stream))

        for _ in range(a.warmup):
            requests()
            inbox()
        torch.cuda.synchronize()
        t_rq, t_ib = [], []
        for _ in range(a.runs):  # interleaved
            t_rq.append(event_ms(requests))
            t_ib.append(event_ms(inbox))
        d = {"records": n, "dispositions": disp, "output_records": int(rq.count.item()),
             "deferred": int(rq.deferred_count.item()),
             "inbox_deferred": int(ib.deferred_count.item()),
             "qe_requests": summary(t_rq), "qe_inbox": summary(t_ib)}
        d["ratio"] = d["qe_requests"]["median_ms"] / d["qe_inbox"]["median_ms"]
        res["lists"][name] = d
        del rq, ib
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
