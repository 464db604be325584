#!/usr/bin/env python3
"""One qe_apply_conf call against the host-row path it replaces, on the
16M-group switch_config state of bench.py with 1 % of the groups in the list
(DESIGN.md §6 holds the figures and the method).

  python scripts/apply_conf_bench.py [--groups G] [--reps N] [--out FILE]

Both paths run in one process on the same state, interleaved A B A B ..., the
state reset before each (not timed).  A timed run starts with the list as
numpy arrays on the host and ends, after a device synchronisation, with the
per-change ConfStates and results on the host:

  list   H2D of the n-record list, qe_apply_conf, D2H of the n records;
  rows   the list scattered into op / count / type / node_id rows [G] on the
         host, H2D of those rows, D2H of state [G], the `switched` row built
         and sent, qe_confchange + qe_switch_config, D2H of the results and of
         the mask rows [G] the ConfState is read from.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import bench
    from etcd_amd import _lib, engine
    bench.engine = engine  # (bench.py imports it in its own main)

    dev = torch.device("cuda:0")
    _, _, S, kind = bench.WORKLOADS["switch_config"]
    G, C = args.groups, 1

    class D:
        rank = 0
    D.dev = dev
    stats = engine.stats_buffer(dev)
    _, _, _, _, keep = bench.setup("switch_config", G, S, kind, D, stats)
    ps, prepare = keep["ps"], keep["prepare"]
    # before the change: voters in slots 0-3, a learner in slot 4, every slot tracked
    cs = engine.ConfState(G, S, dev)
    conf0 = dict(inc=0b01111, out=0, learner=0b10000, learners_next=0, is_learner=0b10000,
                 tracked=0b11111)
    ps.inc, ps.tracked = cs.inc, cs.tracked
    ps.out = cs.out
    ids0 = (torch.arange(S, device=dev, dtype=torch.int64) + 1).repeat_interleave(G)
    fol = engine.Follower(ps)
    fol.state.fill_(_lib.QE_STATE_LEADER)

    def reset():
        prepare()
        for k, v in conf0.items():
            getattr(cs, k).fill_(v)
        cs.auto_leave.zero_()
        cs.slot_ids.copy_(ids0)
        torch.cuda.synchronize()

    # the list: every 100th group; half remove voter 4, half promote learner 5
    groups = np.arange(0, G, 100, dtype=np.uint64)
    n, gi = groups.size, groups.astype(np.int64)
    typ = np.where(np.arange(n) % 2 == 0, _lib.QE_CC_REMOVE_NODE, _lib.QE_CC_ADD_NODE).astype(np.uint8)
    node = np.where(np.arange(n) % 2 == 0, 4, 5).astype(np.uint64)
    trans, cnt = np.zeros(n, np.uint8), np.ones(n, np.uint8)
    ac = engine.ApplyConf(ps, n, max_changes=C, slots=False, ids=False)
    sw = engine.Switch(ps)
    ch = engine.ConfChanges(G, S, C, dev)

    def run_list():
        ac.load_host(group=groups, transition=trans, num_changes=cnt, type=typ, node_id=node)
        engine.apply_conf(ps, fol, cs, ac, sw)
        return ac.records()

    def run_rows():
        op, count = np.zeros(G, np.uint8), np.zeros(G, np.uint8)
        t, nd = np.zeros(G, np.uint8), np.zeros(G, np.uint64)
        op[gi], count[gi], t[gi], nd[gi] = _lib.QE_CC_OP_SIMPLE, cnt, typ, node
        ch.op.copy_(torch.from_numpy(op))
        ch.count.copy_(torch.from_numpy(count))
        ch.type.copy_(torch.from_numpy(t))
        ch.node_id.copy_(torch.from_numpy(nd.view(np.int64)))
        ch.last_index.copy_(ps.last_index)
        state = fol.state.cpu().numpy()
        engine.confchange(cs, ch, ps)
        res = ch.result.cpu().numpy()
        switched = ((res == 0) & (op != 0) & (state == _lib.QE_STATE_LEADER)).astype(np.uint8)
        sw.switched = torch.from_numpy(switched).to(dev)
        engine.switch_config(ps, sw)
        sw.switched = None
        out = {k: getattr(cs, k).cpu().numpy() for k in ("inc", "out", "learner", "learners_next",
                                                         "tracked", "auto_leave")}
        return res, sw.result.cpu().numpy(), out

    def timed(fn):
        reset()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def device_ms():
        """The four kernels of one qe_apply_conf call alone (device events)."""
        reset()
        ac.load_host(group=groups, transition=trans, num_changes=cnt, type=typ, node_id=node)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        engine.apply_conf(ps, fol, cs, ac, sw)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    # the two paths agree before anything is timed
    _, (_, rec) = timed(run_list)
    state_list = {k: getattr(ps, k).clone() for k in ("next", "peer", "committed")}
    sw_list = sw.result.clone()
    _, (res, swres, _) = timed(run_rows)
    assert all(torch.equal(state_list[k], getattr(ps, k)) for k in state_list)
    assert torch.equal(sw_list, sw.result) and (res[gi] == 0).all()
    assert (rec["result"] == _lib.QE_AC_LEADER).all()
    assert (rec["sw_result"] == swres[gi]).all()
    t_list, t_rows, t_dev = [], [], []
    for _ in range(args.reps):
        t_list.append(timed(run_list)[0])
        t_rows.append(timed(run_rows)[0])
        t_dev.append(device_ms())

    def summary(v):
        return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3),
                "max_ms": round(max(v), 3), "runs": len(v)}
    out = {"groups": G, "records": int(n), "slots": S, "device": torch.cuda.get_device_name(0),
           "list": summary(t_list), "rows": summary(t_rows), "list_device_only": summary(t_dev)}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
