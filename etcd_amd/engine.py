"""Device-buffer layer over the C ABI: slot-SoA batches held in HBM as torch
tensors (torch is plumbing here: allocation, streams, distributed), and thin
callers of every qe_* entry point.

Layout: match is [S][stride] uint64 (stored as int64 bits),
masks/bitmaps are uint8 for S <= 8 and uint16 (stored as int16) for S <= 16.
`stride` is rounded up to 64 groups so every slot row starts 512-byte aligned
and the 16-byte vector path is always taken.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import (QeElectionParams, QeElectionState, QeGenParams, QeGroups, QeOutputs,
                   QeReplMsgs, QeReplState, check)

ROW_ALIGN = 64


def mask_torch_dtype(S):
    return torch.uint8 if S <= 8 else torch.int16


def mask_np_dtype(S):
    return np.uint8 if S <= 8 else np.uint16


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _np_u64(t):
    return t.detach().cpu().numpy().view(np.uint64)


class SlotBatch:
    """G Raft groups in slot-SoA form on one device (the qe_groups view)."""

    def __init__(self, G, S, device="cuda", masks=("inc", "out", "learner"), votes=True,
                 group_offset=0, stride=None):
        if not 1 <= S <= _lib.QE_MAX_SLOTS:
            raise ValueError(f"num_slots must be 1..{_lib.QE_MAX_SLOTS}")
        self.G, self.S = int(G), int(S)
        self.device = torch.device(device)
        self.group_offset = int(group_offset)
        self.stride = int(stride) if stride else max(ROW_ALIGN, -(-self.G // ROW_ALIGN) * ROW_ALIGN)
        md = mask_torch_dtype(S)
        dev = self.device
        self.match = torch.zeros(self.S * self.stride, dtype=torch.int64, device=dev)
        self.inc = torch.zeros(self.G, dtype=md, device=dev) if "inc" in masks else None
        self.out = torch.zeros(self.G, dtype=md, device=dev) if "out" in masks else None
        self.learner = torch.zeros(self.G, dtype=md, device=dev) if "learner" in masks else None
        self.voted = torch.zeros(self.G, dtype=md, device=dev) if votes else None
        self.granted = torch.zeros(self.G, dtype=md, device=dev) if votes else None

    # -- views --------------------------------------------------------------
    def struct(self):
        return QeGroups(self.G, self.group_offset, self.S, 0, self.stride, _ptr(self.match),
                        _ptr(self.inc), _ptr(self.out), _ptr(self.learner), _ptr(self.voted),
                        _ptr(self.granted))

    def bytes_per_group(self, with_outputs=True):
        """Algorithmic bytes one qe_commit_vote evaluation moves per group."""
        mb = 1 if self.S <= 8 else 2
        b = 8 * self.S
        b += mb * sum(x is not None for x in (self.inc, self.out, self.learner, self.voted,
                                                self.granted))
        if with_outputs:
            b += 8 + 1
        return b

    def match_rows(self):
        """[S][G] view of the match array."""
        return self.match.view(self.S, self.stride)[:, : self.G]

    # -- host transfer ------------------------------------------------------
    def load_host(self, match, inc=None, out=None, learner=None, voted=None, granted=None):
        """match: uint64 array [S][G] (or [S][stride]); masks: [G] arrays."""
        m = np.ascontiguousarray(np.asarray(match, dtype=np.uint64)).reshape(self.S, -1)
        rows = self.match_rows()
        rows.copy_(torch.from_numpy(m[:, : self.G].view(np.int64).copy()).to(self.device))
        md = mask_np_dtype(self.S)
        for name, arr in (("inc", inc), ("out", out), ("learner", learner), ("voted", voted),
                          ("granted", granted)):
            dst = getattr(self, name)
            if arr is None or dst is None:
                continue
            a = np.ascontiguousarray(np.asarray(arr).astype(md))
            if md == np.uint16:
                a = a.view(np.int16)
            dst.copy_(torch.from_numpy(a).to(self.device))
        return self

    def host(self):
        """Return a dict of numpy arrays (match as [S][G] uint64)."""
        md = mask_np_dtype(self.S)
        out = {"match": self.match_rows().cpu().numpy().view(np.uint64)}
        for name in ("inc", "out", "learner", "voted", "granted"):
            t = getattr(self, name)
            out[name] = None if t is None else t.cpu().numpy().view(md)
        return out


def stats_buffer(device="cuda"):
    return torch.zeros(_lib.QE_STATS_WORDS, dtype=torch.int64, device=device)


def stats_reduce(stats):
    """Fold the shards of a stats buffer on device -> int64[16] tensor."""
    out = torch.empty(_lib.QE_STATS_COUNTERS, dtype=torch.int64, device=stats.device)
    check("qe_stats_reduce", _lib.lib().qe_stats_reduce(_ptr(stats), _ptr(out),
                                                         _stream(stats.device)))
    return out


def collect(flags, values=None, group_offset=0, scratch=None, perm=None):
    """qe_collect: the groups with flags[g] != 0 in ascending position order
    (the Ready-style delta of a batch step, e.g. qe_replication_round's `adv`
    with `committed` as values) -> (groups int64[n], values int64[n] or None).
    perm (device int64[G], qe_pack_order) maps packed positions back to the
    caller's group ids.  One int64 count is read back to size the result."""
    G = flags.numel()
    dev = flags.device
    lib = _lib.lib()
    if scratch is None:
        scratch = torch.empty((lib.qe_collect_scratch_bytes(G) + 7) // 8, dtype=torch.int64,
                              device=dev)
    groups = torch.empty(max(1, G), dtype=torch.int64, device=dev)
    vals = torch.empty(max(1, G), dtype=torch.int64, device=dev) if values is not None else None
    count = torch.empty(1, dtype=torch.int64, device=dev)
    check("qe_collect", lib.qe_collect(G, group_offset, _ptr(perm), _ptr(flags), _ptr(values),
                                       _ptr(groups),
                                       _ptr(vals), _ptr(count), _ptr(scratch), _stream(dev)))
    n = int(count.item())
    return groups[:n], (vals[:n] if vals is not None else None)


def stats_dict(folded):
    v = folded.detach().cpu().numpy().view(np.uint64)
    return {name: int(v[i]) for i, name in enumerate(_lib.STAT_NAMES)}


def gen_groups(batch, seed, dist=0, p_absent=3277, p_voted=52429, p_granted=39322, n_inc=0,
               n_out=0, mask_mode=0, values_only=False):
    """Fill `batch` with the counter-based synthetic generator.
    values_only: Match and votes only, the batch's masks are left as they are
    (e.g. as a packer wrote them)."""
    p = QeGenParams(seed, 0, dist, p_absent, p_voted, p_granted, n_inc, n_out, mask_mode, 0)
    g = batch.struct()
    if values_only:
        g.inc_mask = g.out_mask = g.learner_mask = None
    check("qe_gen_groups", _lib.lib().qe_gen_groups(C.byref(g), C.byref(p),
                                                     _stream(batch.device)))
    return batch


class Outputs:
    def __init__(self, G, device, commit=True, vote=True, tally=True):
        self.commit = torch.empty(G, dtype=torch.int64, device=device) if commit else None
        self.vote = torch.empty(G, dtype=torch.uint8, device=device) if vote else None
        self.granted = torch.empty(G, dtype=torch.uint8, device=device) if tally else None
        self.rejected = torch.empty(G, dtype=torch.uint8, device=device) if tally else None

    def struct(self, stats=None):
        return QeOutputs(_ptr(self.commit), _ptr(self.vote), _ptr(self.granted),
                         _ptr(self.rejected), _ptr(stats))


def commit_vote(batch, outputs=None, stats=None):
    """ProgressTracker.Committed + TallyVotes for every group (qe_commit_vote)."""
    if outputs is None:
        outputs = Outputs(batch.G, batch.device)
    g = batch.struct()
    o = outputs.struct(stats)
    check("qe_commit_vote", _lib.lib().qe_commit_vote(C.byref(g), C.byref(o),
                                                       _stream(batch.device)))
    return outputs


def committed_index(batch, commit=None):
    commit = torch.empty(batch.G, dtype=torch.int64, device=batch.device) if commit is None else commit
    g = batch.struct()
    check("qe_committed_index", _lib.lib().qe_committed_index(C.byref(g), _ptr(commit),
                                                               _stream(batch.device)))
    return commit


def vote_result(batch, vote=None):
    vote = torch.empty(batch.G, dtype=torch.uint8, device=batch.device) if vote is None else vote
    g = batch.struct()
    check("qe_vote_result", _lib.lib().qe_vote_result(C.byref(g), _ptr(vote),
                                                       _stream(batch.device)))
    return vote


def quorum_active(batch, recent_active, active=None):
    active = torch.empty(batch.G, dtype=torch.uint8, device=batch.device) if active is None else active
    g = batch.struct()
    check("qe_quorum_active", _lib.lib().qe_quorum_active(C.byref(g), _ptr(recent_active),
                                                           _ptr(active), _stream(batch.device)))
    return active


def record_votes(batch, resp_mask, resp_value):
    check("qe_record_votes", _lib.lib().qe_record_votes(
        batch.G, batch.S, _ptr(batch.voted), _ptr(batch.granted), _ptr(resp_mask),
        _ptr(resp_value), _stream(batch.device)))


class ReplicationState:
    """Leader-side Progress state of G groups for qe_replication_round."""

    def __init__(self, batch, committed, term_start, last_index, nxt=None):
        self.batch = batch
        self.match = batch.match
        self.next = nxt if nxt is not None else batch.match.clone() + 1
        self.committed = committed
        self.term_start = term_start
        self.last_index = last_index

    def struct(self):
        b = self.batch
        return QeReplState(b.G, b.group_offset, b.S, 0, b.stride, _ptr(self.match),
                           _ptr(self.next), _ptr(self.committed), _ptr(self.term_start),
                           _ptr(self.last_index), _ptr(b.inc), _ptr(b.out))


def replication_round(state, resp_index, resp_mask, read_acks=None, read_ok=None, adv=None,
                      stats=None):
    m = QeReplMsgs(_ptr(resp_index), _ptr(resp_mask), _ptr(read_acks), _ptr(read_ok), _ptr(adv))
    s = state.struct()
    check("qe_replication_round", _lib.lib().qe_replication_round(
        C.byref(s), C.byref(m), _ptr(stats), _stream(state.batch.device)))


class ElectionState:
    """Per-group candidate state for qe_election_steps."""

    def __init__(self, batch, self_slot):
        G, dev = batch.G, batch.device
        self.batch = batch
        self.term = torch.zeros(G, dtype=torch.int64, device=dev)
        self.state = torch.zeros(G, dtype=torch.uint8, device=dev)
        self.voted = torch.zeros(G, dtype=mask_torch_dtype(batch.S), device=dev)
        self.granted = torch.zeros(G, dtype=mask_torch_dtype(batch.S), device=dev)
        self.self_slot = self_slot

    def struct(self):
        b = self.batch
        return QeElectionState(b.G, b.group_offset, b.S, 0, _ptr(self.term), _ptr(self.state),
                               _ptr(self.voted), _ptr(self.granted), _ptr(self.self_slot),
                               _ptr(b.inc), _ptr(b.out), _ptr(b.learner))


def first_voter_slot(batch):
    """self_slot = lowest slot of JointConfig[0] (device computation)."""
    inc = batch.inc.to(torch.int32) & ((1 << batch.S) - 1)
    slot = torch.zeros(batch.G, dtype=torch.uint8, device=batch.device)
    found = torch.zeros(batch.G, dtype=torch.bool, device=batch.device)
    for s in range(batch.S):
        bit = ((inc >> s) & 1).bool() & ~found
        slot = torch.where(bit, torch.full_like(slot, s), slot)
        found |= bit
    return slot


def election_steps(est, seed, step0, steps, p_drop=13107, p_grant=32768, stats=None, flags=0,
                   p_active=0, script=None):
    """script: None or (resp, grant, hup, stride) device tensors [steps][stride]
    (hup may be None) replacing the RNG (qe_election_params scripted mode)."""
    sr, sg, sh, ss = script if script is not None else (None, None, None, 0)
    p = QeElectionParams(seed, step0, steps, p_drop, p_grant, flags, p_active, 0, _ptr(sr),
                         _ptr(sg), _ptr(sh), ss)
    s = est.struct()
    check("qe_election_steps", _lib.lib().qe_election_steps(C.byref(s), C.byref(p), _ptr(stats),
                                                             _stream(est.batch.device)))


def tune(key, value):
    check("qe_tune", _lib.lib().qe_tune(key.encode(), int(value)))


def pack_peer_word(flags, start=0, count=0):
    """The packed per-peer word (include/etcd_quorum.h QE_PW_*): flag bits
    (StateType | ProbeSent << 2 | RecentActive << 3), Inflights.start << 8,
    Inflights.count << 16.  numpy arrays or ints."""
    return ((np.asarray(flags, np.uint32) & 0xF) | (np.asarray(start, np.uint32) << 8) |
            (np.asarray(count, np.uint32) << 16)).astype(np.uint32)


class ProgressState:
    """Device-resident leader-side Progress of G groups (qe_progress):
    match/next/pending [S][stride], the packed per-peer words `peer` [S][stride]
    (int32 storage of the u32 QE_PW_* words), Inflights rings as 32-bit entry
    words `ilo` / `ihi` [S][stride][QE_RING_PITCH(F)] (lane-major, ABI 4: the
    upper words come from the peer word's epoch unless QE_PF_RING_WIDE),
    committed, and the leader-log model (term runs).  `extras`
    allocates the optional per-group arrays: "tracked" (slot mask),
    "self_slot", "lead_transferee" (u8, 0xFF = none), "snap_index" (u64),
    "reads" (ABI 5: the ReadIndex queue -- read_acks [G][QE_READ_QUEUE]
    mask-typed, read_head u32 (starting at context 1), read_count u8; ABI 7:
    read_cap > QE_READ_QUEUE adds the overflow ring read_ovf [G][read_cap]
    mask-typed), "read_keys" (ABI 7: [G][cap] u64 request keys, for
    qe_read_index's duplicate check).  ring16 (ABI 8): the rings in the
    16-bit form, `infl16` [S][stride][8] offsets below Next (F <= 8, S <= 9,
    R <= 4; ilo / ihi then hold the wide peers)."""

    def __init__(self, G, S, F, R, device="cuda", masks=(), group_offset=0, stride=None,
                 extras=(), max_ents=0, read_cap=0, ring16=False):
        if not 1 <= S <= _lib.QE_MAX_SLOTS or not 1 <= F <= _lib.QE_MAX_INFLIGHT:
            raise ValueError("bad num_slots / inflight_cap")
        if not 1 <= R <= _lib.QE_MAX_LOG_RUNS:
            raise ValueError("bad log_runs")
        self.G, self.S, self.F, self.R = int(G), int(S), int(F), int(R)
        self.max_ents = int(max_ents)
        self.device = torch.device(device)
        self.group_offset = int(group_offset)
        self.stride = int(stride) if stride else max(ROW_ALIGN, -(-self.G // ROW_ALIGN) * ROW_ALIGN)
        dev, n = self.device, self.S * self.stride
        i64, u8 = torch.int64, torch.uint8
        self.match = torch.zeros(n, dtype=i64, device=dev)
        self.next = torch.ones(n, dtype=i64, device=dev)
        self.pending = torch.zeros(n, dtype=i64, device=dev)
        self.peer = torch.zeros(n, dtype=torch.int32, device=dev)
        self.FP = _lib.QE_RING_PITCH(self.F)
        self.ilo = torch.zeros(n * self.FP, dtype=torch.int32, device=dev)
        self.ihi = torch.zeros(n * self.FP, dtype=torch.int32, device=dev)
        self.committed = torch.zeros(self.G, dtype=i64, device=dev)
        self.term_start = torch.zeros(self.G, dtype=i64, device=dev)
        self.first_index = torch.ones(self.G, dtype=i64, device=dev)
        self.last_index = torch.zeros(self.G, dtype=i64, device=dev)
        self.run_first = torch.zeros(self.R * self.stride, dtype=i64, device=dev)
        self.run_term = torch.zeros(self.R * self.stride, dtype=i64, device=dev)
        self.run_count = torch.zeros(self.G, dtype=u8, device=dev)
        md = mask_torch_dtype(S)
        self.inc = torch.zeros(self.G, dtype=md, device=dev) if "inc" in masks else None
        self.out = torch.zeros(self.G, dtype=md, device=dev) if "out" in masks else None
        self.tracked = torch.zeros(self.G, dtype=md, device=dev) if "tracked" in extras else None
        self.self_slot = (torch.full((self.G,), 0xFF, dtype=u8, device=dev)
                          if "self_slot" in extras else None)
        self.lead_transferee = (torch.full((self.G,), 0xFF, dtype=u8, device=dev)
                                if "lead_transferee" in extras else None)
        self.snap_index = (torch.zeros(self.G, dtype=i64, device=dev)
                           if "snap_index" in extras else None)
        rq = _lib.QE_READ_QUEUE
        self.read_acks = (torch.zeros(self.G * rq, dtype=md, device=dev)
                          if "reads" in extras else None)
        self.read_head = (torch.ones(self.G, dtype=torch.int32, device=dev)
                          if "reads" in extras else None)
        self.read_count = (torch.zeros(self.G, dtype=u8, device=dev)
                           if "reads" in extras else None)
        self.read_cap = int(read_cap)
        cap = max(rq, self.read_cap)
        self.read_ovf = (torch.zeros(self.G * cap, dtype=md, device=dev)
                         if "reads" in extras and cap > rq else None)
        self.read_keys = (torch.zeros(self.G * cap, dtype=i64, device=dev)
                          if "read_keys" in extras else None)
        if ring16 and (self.F > _lib.QE_RING16_MAX_F or self.S > _lib.QE_RING16_MAX_SLOTS or self.R > 4):
            raise ValueError("the 16-bit Inflights form needs F <= 8, S <= 9, R <= 4")
        self.infl16 = (torch.zeros(n * _lib.QE_RING16_MAX_F, dtype=torch.int16, device=dev)
                       if ring16 else None)

    def struct(self):
        return _lib.QeProgress(
            self.G, self.group_offset, self.S, self.F, self.stride, _ptr(self.match),
            _ptr(self.next), _ptr(self.pending), _ptr(self.peer), _ptr(self.ilo), _ptr(self.ihi),
            _ptr(self.committed), _ptr(self.term_start),
            _ptr(self.first_index), _ptr(self.last_index), self.R, 0, _ptr(self.run_first),
            _ptr(self.run_term), _ptr(self.run_count), _ptr(self.inc), _ptr(self.out),
            _ptr(self.tracked), _ptr(self.self_slot), _ptr(self.lead_transferee),
            _ptr(self.snap_index), self.max_ents, 0, _ptr(self.read_acks), _ptr(self.read_head),
            _ptr(self.read_count), self.read_cap, 0, _ptr(self.read_ovf), _ptr(self.read_keys),
            _ptr(self.infl16))

    ARRAYS = ("match", "next", "pending", "peer", "ilo", "ihi", "committed",
              "term_start", "first_index", "last_index", "run_first", "run_term", "run_count",
              "inc", "out", "tracked", "self_slot", "lead_transferee", "snap_index",
              "read_acks", "read_head", "read_count", "read_ovf", "read_keys", "infl16")

    def load_host(self, **arrays):
        """numpy arrays (uint64 as uint64, masks as uint8/uint16, peer words
        as uint32).  flags / istart / icount (uint8 arrays, any subset) are
        packed into the peer words (absent fields 0).  `ibuf` takes plain
        uint64 Inflights rings, entry-major [S][F][stride] (the oracle's
        layout), converted through qe_ring_pack after the peer words are in
        place (their ring representation bits are recomputed).  Without
        `ibuf`, rewritten peer words keep describing the resident rings: the
        rings are decoded with the old words and packed again with the new
        ones (a new Inflights.start / count selects other live entries) --
        unless raw `ilo` / `ihi` words are passed too, which are then taken
        as they are."""
        ibuf = arrays.pop("ibuf", None)
        fields = {k: arrays.pop(k) for k in ("flags", "istart", "icount") if k in arrays}
        raw_rings = "ilo" in arrays or "ihi" in arrays or "infl16" in arrays  # the caller's words stand
        # (the 16-bit form's entries are offsets below Next: a new Next re-bases them)
        rebase = fields or "peer" in arrays or (self.infl16 is not None and "next" in arrays)
        if ibuf is None and not raw_rings and rebase:
            ibuf = self.rings()  # decoded with the words (and Next) in place now
        if fields:
            n = max(np.asarray(v).size for v in fields.values())
            z = np.zeros(n, np.uint32)
            arrays["peer"] = pack_peer_word(fields.get("flags", z), fields.get("istart", z),
                                            fields.get("icount", z))
        for k, a in arrays.items():
            dst = getattr(self, k)
            if dst is None or a is None:
                continue
            a = np.ascontiguousarray(a)
            if a.dtype == np.uint64:
                a = a.view(np.int64)
            elif a.dtype == np.uint16:
                a = a.view(np.int16)
            elif a.dtype == np.uint32:
                a = a.view(np.int32)
            a = a.reshape(-1)[: dst.numel()]
            dst[: a.size].copy_(torch.from_numpy(a.copy()).to(self.device))
        if ibuf is not None:
            self.load_rings(ibuf)
        if "pending" in arrays or "peer" in arrays:
            self.check_pending_precondition()
        return self

    def check_pending_precondition(self):
        """The ABI's precondition (include/etcd_quorum.h qe_progress.
        pending_snapshot): PendingSnapshot is 0 for every peer not in
        StateSnapshot -- ResetState clears it on each state change
        (raft/tracker/progress.go:84-89), and the kernels write it only where
        its value changes.  Raises ValueError on a host-loaded state that
        violates it (results would be unspecified)."""
        pend = self.pending.view(self.S, self.stride)[:, : self.G].cpu().numpy()
        state = self.peer.view(self.S, self.stride)[:, : self.G].cpu().numpy() & 3
        bad = (pend != 0) & (state != _lib.QE_PR_SNAPSHOT)
        if bad.any():
            s, g = (int(x[0]) for x in np.nonzero(bad))
            raise ValueError(f"PendingSnapshot != 0 outside StateSnapshot (slot {s}, group {g}): "
                             "the qe_progress precondition")

    def load_rings(self, ibuf):
        """Plain uint64 rings, entry-major [S][F][stride] -> ilo / ihi and the
        peer words' representation bits (qe_ring_pack, host side)."""
        S, F, st = self.S, self.F, self.stride
        e = np.zeros(S * F * st, np.uint64)
        a = np.asarray(ibuf, np.uint64).reshape(-1)[: e.size]
        e[: a.size] = a
        ent = np.ascontiguousarray(e.reshape(S, F, st).transpose(0, 2, 1))  # [S][stride][F]
        peer = self.peer.cpu().numpy().view(np.uint32).copy()
        lo = np.zeros(S * st * self.FP, np.uint32)
        hi = np.zeros_like(lo)
        if self.infl16 is not None:  # ABI 8: offsets below Next, wide where they do not fit
            nxt = self.next.cpu().numpy().view(np.uint64).copy()
            o16 = np.zeros(S * st * _lib.QE_RING16_MAX_F, np.uint16)
            check("qe_ring_pack16", _lib.lib().qe_ring_pack16(
                self.G, S, F, st, ent.ctypes.data, nxt.ctypes.data, peer.ctypes.data,
                o16.ctypes.data, lo.ctypes.data, hi.ctypes.data))
            self.infl16.copy_(torch.from_numpy(o16.view(np.int16)).to(self.device))
        else:
            check("qe_ring_pack", _lib.lib().qe_ring_pack(
                self.G, S, F, st, ent.ctypes.data, peer.ctypes.data, lo.ctypes.data, hi.ctypes.data))
        for dst, v in ((self.peer, peer), (self.ilo, lo), (self.ihi, hi)):
            dst.copy_(torch.from_numpy(v.view(np.int32)).to(self.device))

    def set_ring_slot(self, s, ent):
        """Slot s's rings from a device int64 tensor [stride][F] (uint64
        entries), in place on the device: the 32-bit words, and the peer
        words' representation bits in canonical form (the rule of
        qe_ring_pack) from their Inflights.start / count."""
        S, F, st, FP = self.S, self.F, self.stride, self.FP
        ent = ent.view(st, F)
        lo = ent & 0xFFFFFFFF
        hi = (ent >> 32) & 0xFFFFFFFF
        as_i32 = lambda v: torch.where(v >= (1 << 31), v - (1 << 32), v).to(torch.int32)  # noqa: E731
        rows = slice(s * st, (s + 1) * st)
        self.ilo.view(S * st, FP)[rows, :F] = as_i32(lo)
        self.ihi.view(S * st, FP)[rows, :F] = as_i32(hi)
        w = self.peer[rows].to(torch.int64) & 0xFFFFFFFF
        start, count = (w >> 8) & 0xFF, (w >> 16) & 0xFF
        k = torch.arange(F, device=self.device).view(1, F)
        live = torch.remainder(k - start.view(st, 1), F) < count.view(st, 1)
        if self.infl16 is not None:  # ABI 8: offsets below Next (the rule of qe_ring_pack16)
            top = (self.next[rows] - 1).view(st, 1)
            d = top - ent  # int64; entries and Next below 2^63 here
            off = d & 0xFFFF
            fits = ((d >= 0) & (d <= 0xFFFF)) | ~live
            o = torch.zeros(st, _lib.QE_RING16_MAX_F, dtype=torch.int64, device=self.device)
            o[:, :F] = off
            self.infl16.view(S * st, _lib.QE_RING16_MAX_F)[rows] = torch.where(
                o >= (1 << 15), o - (1 << 16), o).to(torch.int16)
            rep = torch.where(fits.all(1), 0, _lib.QE_PF_RING_WIDE)
            w = (w & ~_lib.QE_PW_RING_MASK & 0xFFFFFFFF) | rep
            self.peer[rows] = as_i32(w)
            return
        hmin = torch.where(live, hi, 1 << 40).amin(1)
        hmax = torch.where(live, hi, -1).amax(1)
        uni = (hmin == hmax) & (hmax <= _lib.QE_RING_EPOCH_MAX)
        h = torch.where(uni, hmin, 0)
        ep_bits = ((h & 7) << 5) | ((h & 0x7F8) << 21)
        rep = torch.where(count == 0, 0, torch.where(uni, ep_bits, _lib.QE_PF_RING_WIDE))
        w = (w & ~_lib.QE_PW_RING_MASK & 0xFFFFFFFF) | rep
        self.peer[rows] = as_i32(w)

    def rings(self, peer=None):
        """Every ring position decoded to uint64 (qe_ring_unpack), entry-major
        [S][F][stride] flattened (groups >= G are 0)."""
        S, F, st = self.S, self.F, self.stride
        if peer is None:
            peer = self.peer.cpu().numpy().view(np.uint32)
        lo = self.ilo.cpu().numpy().view(np.uint32)
        hi = self.ihi.cpu().numpy().view(np.uint32)
        ent = np.zeros(S * st * F, np.uint64)
        if self.infl16 is not None:  # ABI 8
            o16 = self.infl16.cpu().numpy().view(np.uint16)
            nxt = self.next.cpu().numpy().view(np.uint64)
            check("qe_ring_unpack16", _lib.lib().qe_ring_unpack16(
                self.G, S, F, st, o16.ctypes.data, lo.ctypes.data, hi.ctypes.data,
                nxt.ctypes.data, np.ascontiguousarray(peer).ctypes.data, ent.ctypes.data))
        else:
            check("qe_ring_unpack", _lib.lib().qe_ring_unpack(
                self.G, S, F, st, lo.ctypes.data, hi.ctypes.data,
                np.ascontiguousarray(peer).ctypes.data, ent.ctypes.data))
        return np.ascontiguousarray(ent.reshape(S, st, F).transpose(0, 2, 1)).reshape(-1)

    def host(self):
        out = {}
        for k in self.ARRAYS:
            t = getattr(self, k)
            if t is None:
                out[k] = None
                continue
            a = t.cpu().numpy()
            out[k] = a.view(np.uint64) if a.dtype == np.int64 else (
                a.view(np.uint16) if a.dtype == np.int16 else (
                    a.view(np.uint32) if a.dtype == np.int32 else a))
        w = out["peer"]
        out["ibuf"] = self.rings(w)
        out["flags"] = (w & 0xF).astype(np.uint8)
        out["istart"] = ((w >> 8) & 0xFF).astype(np.uint8)
        out["icount"] = ((w >> 16) & 0xFF).astype(np.uint8)
        return out


class PeerMsgs:
    """One round of per-peer messages for qe_progress_step ([S][stride]) and
    its outputs (sent / snap / timeout_now masks and bcast count per group,
    msg_count / msg_index per peer)."""

    def __init__(self, ps, outputs=True):
        dev, n = ps.device, ps.S * ps.stride
        md = mask_torch_dtype(ps.S)
        self.type = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.index = torch.zeros(n, dtype=torch.int64, device=dev)
        self.reject_hint = torch.zeros(n, dtype=torch.int64, device=dev)
        self.log_term = torch.zeros(n, dtype=torch.int64, device=dev)
        self.sent = torch.zeros(ps.G, dtype=md, device=dev) if outputs else None
        self.bcast = torch.zeros(ps.G, dtype=torch.uint8, device=dev) if outputs else None
        self.snap = torch.zeros(ps.G, dtype=md, device=dev) if outputs else None
        self.timeout_now = torch.zeros(ps.G, dtype=md, device=dev) if outputs else None
        self.msg_count = torch.zeros(n, dtype=torch.uint8, device=dev) if outputs else None
        self.msg_index = torch.zeros(n, dtype=torch.int64, device=dev) if outputs else None
        self.bytes_requested = None
        # ReadIndex (ABI 5): contexts carried by heartbeat responses (None =
        # the newest pending at the start of the round) and the outputs
        self.read_ctx = None       # [S][stride] uint32 (int32 storage)
        self.read_released = torch.zeros(ps.G, dtype=torch.uint8, device=dev) if outputs else None
        self.term_commit = torch.zeros(ps.G, dtype=torch.uint8, device=dev) if outputs else None
        self.term_commit_index = (torch.zeros(ps.G, dtype=torch.int64, device=dev)
                                  if outputs else None)

    def set_read_ctx(self, ps, ctx):
        """Context numbers of the heartbeat responses: uint32 [S][stride]
        (numpy or tensor); None = every response carries the newest context
        pending when the round starts."""
        if ctx is None:
            self.read_ctx = None
            return self
        if not torch.is_tensor(ctx):
            a = np.ascontiguousarray(np.asarray(ctx, np.uint32)).view(np.int32)
            ctx = torch.from_numpy(a.copy())
        t = torch.zeros(ps.S * ps.stride, dtype=torch.int32, device=ps.device)
        t[: ctx.numel()].copy_(ctx.reshape(-1).to(torch.int32))
        self.read_ctx = t
        return self

    def struct(self):
        return _lib.QePeerMsgs(_ptr(self.type), _ptr(self.index), _ptr(self.reject_hint),
                               _ptr(self.log_term), _ptr(self.sent), _ptr(self.bcast),
                               _ptr(self.snap), _ptr(self.timeout_now), _ptr(self.msg_count),
                               _ptr(self.msg_index), _ptr(self.bytes_requested),
                               _ptr(self.read_ctx), _ptr(self.read_released),
                               _ptr(self.term_commit), _ptr(self.term_commit_index))


def progress_step(ps, msgs, stats=None):
    p, m = ps.struct(), msgs.struct()
    check("qe_progress_step", _lib.lib().qe_progress_step(C.byref(p), C.byref(m), _ptr(stats),
                                                           _stream(ps.device)))


def progress_bytes_requested(ps, msgs):
    """Run one round through the instrumented kernel variant and return the
    bytes it requested (reads + writes at field granularity): the
    algorithmic bytes of that round.  Mutates the state like progress_step."""
    acct = torch.zeros(1, dtype=torch.int64, device=ps.device)
    msgs.bytes_requested = acct
    try:
        progress_step(ps, msgs)
    finally:
        msgs.bytes_requested = None
    return int(acct.item())


def progress_send(ps, want, send_if_empty=False):
    """qe_progress_send: MaxSizePerMsg is ps.max_ents (ABI 3)."""
    sent = torch.zeros(ps.G, dtype=mask_torch_dtype(ps.S), device=ps.device)
    snap = torch.zeros(ps.G, dtype=mask_torch_dtype(ps.S), device=ps.device)
    p = ps.struct()
    check("qe_progress_send", _lib.lib().qe_progress_send(
        C.byref(p), _ptr(want), int(bool(send_if_empty)), _ptr(sent), _ptr(snap),
        _stream(ps.device)))
    return sent, snap


def read_index(ps, request, lease_based=False, key=None):
    """qe_read_index: MsgReadIndex on the leader of every group with
    request[g] != 0 (raft/raft.go:1078-1096) -> (result uint8[G] QE_RI_*,
    ctx int32[G] (the context number of a QUEUED request, or of the pending
    one a DUPLICATE key names), index int64[G] (the read index of RESPOND /
    QUEUED)).  key: int64[G] request keys (ABI 7, with ps.read_keys)."""
    G, dev = ps.G, ps.device
    result = torch.zeros(G, dtype=torch.uint8, device=dev)
    ctx = torch.zeros(G, dtype=torch.int32, device=dev)
    index = torch.zeros(G, dtype=torch.int64, device=dev)
    p = ps.struct()
    check("qe_read_index", _lib.lib().qe_read_index(
        C.byref(p), _ptr(request), _ptr(key), int(bool(lease_based)), _ptr(result), _ptr(ctx),
        _ptr(index),
        _stream(dev)))
    return result, ctx, index


def check_quorum(ps, quorum_active=None, stats=None):
    """qe_check_quorum: MsgCheckQuorum on every group's leader
    (raft/raft.go:997-1018) over the resident Progress words -> uint8[G]
    QuorumActive (0 = the leader steps down)."""
    if quorum_active is None:
        quorum_active = torch.empty(ps.G, dtype=torch.uint8, device=ps.device)
    p = ps.struct()
    check("qe_check_quorum", _lib.lib().qe_check_quorum(C.byref(p), _ptr(quorum_active),
                                                         _ptr(stats), _stream(ps.device)))
    return quorum_active


def heartbeat(ps, commit=None, ctx=None, sent=None):
    """qe_heartbeat: MsgBeat -> bcastHeartbeat (raft/raft.go:524-541) ->
    (commit int64 [S][stride]: min(Match, committed) of every slot sent to,
    ctx int32 [G]: the newest pending ReadIndex context, sent mask [G])."""
    if commit is None:
        commit = torch.zeros(ps.S * ps.stride, dtype=torch.int64, device=ps.device)
    if ctx is None:
        ctx = torch.zeros(ps.G, dtype=torch.int32, device=ps.device)
    if sent is None:
        sent = torch.zeros(ps.G, dtype=mask_torch_dtype(ps.S), device=ps.device)
    p = ps.struct()
    check("qe_heartbeat", _lib.lib().qe_heartbeat(C.byref(p), _ptr(commit), _ptr(ctx), _ptr(sent),
                                                   _stream(ps.device)))
    return commit, ctx, sent


class Timers:
    """Device-resident tick state of G groups (qe_timers): `state` u8
    QE_STATE_*, `timer` int32 storage of electionElapsed | heartbeatElapsed
    << 16, `randomized_timeout` int16 storage of the u16
    randomizedElectionTimeout, `no_campaign` u8 (hasPendingSnapshot),
    `events` u8 QE_TEV_* (cleared by the tick() that consumes them).
    check_quorum is raft.Config.CheckQuorum; `tick_no` counts the ticks run
    and is the counter of the timeout draw."""

    def __init__(self, G, election_timeout=10, heartbeat_timeout=1, check_quorum=False,
                 seed=0, device="cuda", tick_no=0):
        if not 1 <= int(election_timeout) <= 32768 or not 1 <= int(heartbeat_timeout) <= 65535:
            raise ValueError("election_timeout must be 1..32768, heartbeat_timeout 1..65535")
        self.G = int(G)
        self.device = torch.device(device)
        self.election_timeout, self.heartbeat_timeout = int(election_timeout), int(heartbeat_timeout)
        self.check_quorum = bool(check_quorum)
        self.seed, self.tick_no = int(seed), int(tick_no)
        dev = self.device
        self.state = torch.zeros(self.G, dtype=torch.uint8, device=dev)
        self.timer = torch.zeros(self.G, dtype=torch.int32, device=dev)
        et = self.election_timeout
        self.randomized_timeout = torch.full((self.G,), et if et < 32768 else et - 65536,
                                             dtype=torch.int16, device=dev)
        self.no_campaign = torch.zeros(self.G, dtype=torch.uint8, device=dev)
        self.events = torch.zeros(self.G, dtype=torch.uint8, device=dev)

    ARRAYS = ("state", "timer", "randomized_timeout", "no_campaign", "events")

    def load_host(self, **arrays):
        """numpy arrays: state / no_campaign / events uint8, timer uint32,
        randomized_timeout uint16; election_elapsed / heartbeat_elapsed (any
        integers, clipped to the counters' 65535) are packed into timer."""
        if "election_elapsed" in arrays or "heartbeat_elapsed" in arrays:
            ee = np.minimum(np.asarray(arrays.pop("election_elapsed", 0), np.int64), 0xFFFF)
            he = np.minimum(np.asarray(arrays.pop("heartbeat_elapsed", 0), np.int64), 0xFFFF)
            arrays["timer"] = np.broadcast_to(ee | (he << 16), (self.G,)).astype(np.uint32)
        for k, a in arrays.items():
            if k not in self.ARRAYS:
                raise KeyError(k)
            a = np.ascontiguousarray(a)
            if a.dtype == np.uint32:
                a = a.view(np.int32)
            elif a.dtype == np.uint16:
                a = a.view(np.int16)
            getattr(self, k).copy_(torch.from_numpy(a.copy()).to(self.device))
        return self

    def reset(self, mask):
        """The timer part of raft.reset() (becomeFollower / Candidate /
        Leader) on the groups of `mask` (bool tensor [G]): applied by the
        next tick() as QE_TEV_RESET."""
        self.events[mask.to(self.device)] |= _lib.QE_TEV_RESET
        return self

    def heard(self, mask):
        """electionElapsed = 0 on the groups of `mask` (QE_TEV_HEARD)."""
        self.events[mask.to(self.device)] |= _lib.QE_TEV_HEARD
        return self

    def struct(self, events=None, ticks=1):
        return _lib.QeTimers(_ptr(self.state), _ptr(self.timer), _ptr(self.randomized_timeout),
                             _ptr(self.no_campaign), _ptr(events), self.election_timeout,
                             self.heartbeat_timeout,
                             _lib.QE_TICK_CHECK_QUORUM if self.check_quorum else 0, int(ticks),
                             self.seed, self.tick_no)

    def host(self):
        out = {k: getattr(self, k).cpu().numpy() for k in self.ARRAYS}
        out["timer"] = out["timer"].view(np.uint32)
        out["randomized_timeout"] = out["randomized_timeout"].view(np.uint16)
        return out


class TickOut:
    """Outputs of qe_tick (qe_tick_out): `action` u8 QE_TICK_*, and where a
    group beat / was checked: hb_commit int64 [S][stride], hb_ctx int32 [G],
    hb_sent mask [G], quorum_active u8 [G]."""

    def __init__(self, ps, beats=True):
        dev = ps.device
        self.action = torch.zeros(ps.G, dtype=torch.uint8, device=dev)
        self.hb_commit = (torch.zeros(ps.S * ps.stride, dtype=torch.int64, device=dev)
                          if beats else None)
        self.hb_ctx = torch.zeros(ps.G, dtype=torch.int32, device=dev) if beats else None
        self.hb_sent = torch.zeros(ps.G, dtype=mask_torch_dtype(ps.S), device=dev)
        self.quorum_active = torch.zeros(ps.G, dtype=torch.uint8, device=dev)

    def struct(self):
        return _lib.QeTickOut(_ptr(self.action), _ptr(self.hb_commit), _ptr(self.hb_ctx),
                              _ptr(self.hb_sent), _ptr(self.quorum_active))


def tick(ps, timers, out=None, stats=None, events=None, ticks=1):
    """qe_tick: raft.tick() on every group -- tickElection / tickHeartbeat
    (raft/raft.go:645-684) over the resident timers, with the MsgCheckQuorum
    and MsgBeat they fire run in the same pass -> TickOut.  events (uint8[G]
    QE_TEV_*) default to timers.events, which are consumed (cleared) by the
    call; ticks=0 applies the events alone."""
    if out is None:
        out = TickOut(ps)
    own = events is None
    if own:
        events = timers.events
    p, t, o = ps.struct(), timers.struct(events, ticks), out.struct()
    check("qe_tick", _lib.lib().qe_tick(C.byref(p), C.byref(t), C.byref(o), _ptr(stats),
                                         _stream(ps.device)))
    if own:
        timers.events.zero_()
    timers.tick_no += int(ticks)
    return out


_SIGNED = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32,
           np.dtype(np.uint16): np.int16}


class _Rows:
    """A bundle of device rows described by FIELDS, "name:kind" words with
    kind u8, u32, u64 (int32 / int64 storage) or mask (u8, or int16 storage of
    u16); a trailing "?" marks a row the constructor may leave out (None).
    load_host(**arrays) copies numpy arrays of the unsigned types in (`from`
    is accepted for `from_`; an array for a row that was left out is dropped);
    host() returns the rows of HOST (default: all) as numpy arrays of the
    unsigned types, None for a row left out."""

    FIELDS = ""

    def __init_subclass__(cls):
        words = [w.rstrip("?").split(":") for w in cls.FIELDS.split()]
        cls.ARRAYS, cls.KIND = tuple(w[0] for w in words), dict(words)
        cls.HOST = cls.__dict__.get("HOST", cls.ARRAYS)  # (a base's HOST is its own)

    def load_host(self, **arrays):
        for k, a in arrays.items():
            k = "from_" if k == "from" else k
            if k not in self.ARRAYS:
                raise KeyError(k)
            dst = getattr(self, k)
            if dst is None:
                continue
            a = np.ascontiguousarray(a)
            a = a.view(_SIGNED.get(a.dtype, a.dtype)).reshape(-1)
            dst[: a.size].copy_(torch.from_numpy(a.copy()).to(dst.device))
        return self

    def host(self):
        out = {}
        for k in self.HOST:
            t = getattr(self, k)
            a = None if t is None else t.cpu().numpy()
            kind = {"u64": np.uint64, "u32": np.uint32, "u8": np.uint8}.get(self.KIND[k])
            if a is not None:  # (a mask row is u8 up to 8 slots, u16 above)
                a = a.view(kind or (np.uint8 if a.dtype == np.uint8 else np.uint16))
            out[k] = a
        return out


_TORCH = {"u8": torch.uint8, "u32": torch.int32, "u64": torch.int64}


class _Records(_Rows):
    """What the record lists of qe_outbox, qe_replies, qe_ready and
    qe_read_states share: rows of max(1, capacity) records allocated from
    FIELDS, the rows named in RUNS as [E][capacity] term runs (left out with
    E = 0), `count` (int64[1]), the cached scratch of the call, and records()."""

    RUNS = ()

    def _alloc(self, device, capacity, runs=0, without=()):
        self.capacity = int(capacity)
        n = max(1, self.capacity)
        for k in self.ARRAYS:
            size = 1 if k == "count" else runs * n if k in self.RUNS else n
            setattr(self, k, None if k in without or not size else
                    torch.zeros(size, dtype=_TORCH[self.KIND[k]], device=device))
        self.scratch = None

    def records(self):
        """-> (count, the rows cut to min(count, capacity) as numpy arrays:
        the run rows as [E][n], None for a row left out)."""
        count = int(self.count.item())
        n, cap = min(count, self.capacity), max(1, self.capacity)
        out = {k: a for k, a in self.host().items() if k != "count"}
        for k, a in out.items():
            if a is not None:
                out[k] = a.reshape(-1, cap)[:, :n] if k in self.RUNS else a[:n]
        return count, out


def _scratch(obj, device, need, grow=0):
    """The scratch tensor cached in `obj` for a call that needs `need` bytes,
    allocated with max(need, grow) bytes when there is none or it is too small."""
    if obj.scratch is None or obj.scratch.numel() * 8 < need:
        obj.scratch = torch.empty((max(need, grow) + 7) // 8 + 1, dtype=torch.int64, device=device)
    return obj.scratch


class Follower(_Rows):
    """Device-resident receiver state of G groups (qe_follower): `term` int64
    storage of r.Term, `state` u8 QE_STATE_* (pass a Timers' `state` tensor to
    share the row with qe_tick), `lead` and `vote` u8 slots (0xFF = None;
    vote=False leaves the row out).  check_quorum / prevote are the raft.Config
    switches that make a lower-term MsgApp / MsgHeartbeat answered."""

    FIELDS = "term:u64 state:u8 lead:u8 vote:u8?"

    def __init__(self, ps, state=None, vote=True, check_quorum=False, prevote=False):
        dev, u8 = ps.device, torch.uint8
        self.term = torch.zeros(ps.G, dtype=torch.int64, device=dev)
        self.state = state if state is not None else torch.zeros(ps.G, dtype=u8, device=dev)
        self.lead = torch.full((ps.G,), 0xFF, dtype=u8, device=dev)
        self.vote = torch.full((ps.G,), 0xFF, dtype=u8, device=dev) if vote else None
        self.flags = ((_lib.QE_FOLLOW_CHECK_QUORUM if check_quorum else 0) |
                      (_lib.QE_FOLLOW_PREVOTE if prevote else 0))

    def struct(self):
        return _lib.QeFollower(_ptr(self.term), _ptr(self.state), _ptr(self.lead),
                               _ptr(self.vote), self.flags, 0)


class LeaderMsgs(_Rows):
    """One MsgApp / MsgHeartbeat per group for qe_follower_step
    (qe_leader_msgs): type / from_ u8, term / index / log_term / commit int64
    storage of the u64 fields, and the entries of a MsgApp as msg_runs term
    runs: ent_len int32 [E][stride], ent_term int64 [E][stride]."""

    FIELDS = ("type:u8 from_:u8 term:u64 index:u64 log_term:u64 commit:u64 ent_len:u32? "
              "ent_term:u64?")

    def __init__(self, ps, msg_runs=1):
        if not 0 <= int(msg_runs) <= _lib.QE_MAX_MSG_RUNS:
            raise ValueError("msg_runs must be 0..QE_MAX_MSG_RUNS")
        dev, i64, u8 = ps.device, torch.int64, torch.uint8
        self.msg_runs = int(msg_runs)
        self.type = torch.zeros(ps.G, dtype=u8, device=dev)
        self.from_ = torch.zeros(ps.G, dtype=u8, device=dev)
        self.term = torch.zeros(ps.G, dtype=i64, device=dev)
        self.index = torch.zeros(ps.G, dtype=i64, device=dev)
        self.log_term = torch.zeros(ps.G, dtype=i64, device=dev)
        self.commit = torch.zeros(ps.G, dtype=i64, device=dev)
        n = self.msg_runs * ps.stride
        self.ent_len = torch.zeros(n, dtype=torch.int32, device=dev) if n else None
        self.ent_term = torch.zeros(n, dtype=i64, device=dev) if n else None

    def struct(self):
        return _lib.QeLeaderMsgs(_ptr(self.type), _ptr(self.from_), _ptr(self.term),
                                 _ptr(self.index), _ptr(self.log_term), _ptr(self.commit),
                                 self.msg_runs, 0, _ptr(self.ent_len), _ptr(self.ent_term))


class FollowerOut(_Rows):
    """Outputs of qe_follower_step (qe_follower_out): `result` u8 QE_FR_*,
    resp_index / reject_hint / resp_log_term / append_from int64 [G], and
    `events` u8 QE_TEV_* [G], written for every group, which tick(...,
    events=) takes as it is."""

    FIELDS = "result:u8 resp_index:u64 reject_hint:u64 resp_log_term:u64 append_from:u64 events:u8"

    def __init__(self, ps):
        dev, i64, u8 = ps.device, torch.int64, torch.uint8
        self.result = torch.zeros(ps.G, dtype=u8, device=dev)
        self.resp_index = torch.zeros(ps.G, dtype=i64, device=dev)
        self.reject_hint = torch.zeros(ps.G, dtype=i64, device=dev)
        self.resp_log_term = torch.zeros(ps.G, dtype=i64, device=dev)
        self.append_from = torch.zeros(ps.G, dtype=i64, device=dev)
        self.events = torch.zeros(ps.G, dtype=u8, device=dev)

    def struct(self):
        return _lib.QeFollowerOut(_ptr(self.result), _ptr(self.resp_index),
                                  _ptr(self.reject_hint), _ptr(self.resp_log_term),
                                  _ptr(self.append_from), _ptr(self.events))


def follower_step(ps, fol, msgs, out=None, stats=None):
    """qe_follower_step: one MsgApp / MsgHeartbeat per group through
    raft.Step's term preamble, handleAppendEntries and handleHeartbeat on the
    log rows of `ps` (committed, last_index, the term runs) -> FollowerOut."""
    if out is None:
        out = FollowerOut(ps)
    p, f, m, o = ps.struct(), fol.struct(), msgs.struct(), out.struct()
    check("qe_follower_step",
          _lib.lib().qe_follower_step(C.byref(p), C.byref(f), C.byref(m), C.byref(o),
                                      _ptr(stats), _stream(ps.device)))
    return out


class Voter(_Rows):
    """The election side of G groups (qe_voter): the Votes map as `voted` /
    `granted` masks [G] (votes=False leaves them out: a voter-only launch,
    which answers requests and refuses responses and campaigns), `no_campaign`
    u8 [G] (pass a Timers' row to share it) and `timer`, the Timers' row the
    lease reads.  Pass `timers` to take timer, no_campaign, election_timeout
    and check_quorum from it."""

    FIELDS = "voted:mask? granted:mask? no_campaign:u8?"
    HOST = ("voted", "granted")

    def __init__(self, ps, timers=None, votes=True, check_quorum=None, prevote=False,
                 election_timeout=None, no_campaign=None):
        dev, md = ps.device, mask_torch_dtype(ps.S)
        self.timer = timers.timer if timers is not None else None
        if no_campaign is None and timers is not None:
            no_campaign = timers.no_campaign
        self.no_campaign = no_campaign
        if election_timeout is None:
            election_timeout = timers.election_timeout if timers is not None else 10
        self.election_timeout = int(election_timeout)
        if check_quorum is None:
            check_quorum = timers.check_quorum if timers is not None else False
        self.flags = ((_lib.QE_VOTE_CHECK_QUORUM if check_quorum else 0) |
                      (_lib.QE_VOTE_PREVOTE if prevote else 0))
        self.voted = torch.zeros(ps.G, dtype=md, device=dev) if votes else None
        self.granted = torch.zeros(ps.G, dtype=md, device=dev) if votes else None

    def struct(self):
        return _lib.QeVoter(_ptr(self.timer), self.election_timeout, self.flags, _ptr(self.voted),
                            _ptr(self.granted), _ptr(self.no_campaign))


class VoteMsgs(_Rows):
    """One election message per group for qe_vote_step (qe_vote_msgs): type
    (QE_VMSG_*) / from_ / flags (QE_VMF_*) u8, term / index / log_term int64
    storage of the u64 fields."""

    FIELDS = "type:u8 from_:u8 term:u64 index:u64 log_term:u64 flags:u8"

    def __init__(self, ps):
        dev, i64, u8 = ps.device, torch.int64, torch.uint8
        self.type = torch.zeros(ps.G, dtype=u8, device=dev)
        self.from_ = torch.zeros(ps.G, dtype=u8, device=dev)
        self.term = torch.zeros(ps.G, dtype=i64, device=dev)
        self.index = torch.zeros(ps.G, dtype=i64, device=dev)
        self.log_term = torch.zeros(ps.G, dtype=i64, device=dev)
        self.flags = torch.zeros(ps.G, dtype=u8, device=dev)

    def struct(self):
        return _lib.QeVoteMsgs(_ptr(self.type), _ptr(self.from_), _ptr(self.term),
                               _ptr(self.index), _ptr(self.log_term), _ptr(self.flags))


class VoteOut(_Rows):
    """Outputs of qe_vote_step (qe_vote_out): `result` u8 QE_VR_*, resp_term /
    req_log_term int64 [G], req_to mask [G], and two rows written for every
    group: `elected` u8, which Leader(ps, elected=) takes as it is, and
    `events` u8 QE_TEV_*, which tick(..., events=) takes as it is."""

    FIELDS = "result:u8 resp_term:u64 req_log_term:u64 req_to:mask elected:u8 events:u8"

    def __init__(self, ps):
        dev, i64, u8 = ps.device, torch.int64, torch.uint8
        self.result = torch.zeros(ps.G, dtype=u8, device=dev)
        self.resp_term = torch.zeros(ps.G, dtype=i64, device=dev)
        self.req_log_term = torch.zeros(ps.G, dtype=i64, device=dev)
        self.req_to = torch.zeros(ps.G, dtype=mask_torch_dtype(ps.S), device=dev)
        self.elected = torch.zeros(ps.G, dtype=u8, device=dev)
        self.events = torch.zeros(ps.G, dtype=u8, device=dev)

    def struct(self):
        return _lib.QeVoteOut(_ptr(self.result), _ptr(self.resp_term), _ptr(self.req_log_term),
                              _ptr(self.req_to), _ptr(self.elected), _ptr(self.events))


def vote_step(ps, fol, voter, msgs, out=None, stats=None):
    """qe_vote_step: one MsgVote / MsgPreVote / response / MsgHup /
    MsgTimeoutNow per group through raft.Step's term preamble and lease, the
    vote decision, the candidate's tally and campaign() on the resident state
    -> VoteOut.  After a QE_VR_WON: become_leader with Leader(ps,
    elected=out.elected) and the Follower's term row."""
    if out is None:
        out = VoteOut(ps)
    p, f, v, m, o = ps.struct(), fol.struct(), voter.struct(), msgs.struct(), out.struct()
    check("qe_vote_step",
          _lib.lib().qe_vote_step(C.byref(p), C.byref(f), C.byref(v), C.byref(m), C.byref(o),
                                  _ptr(stats), _stream(ps.device)))
    return out


class Compaction(_Rows):
    """One CreateSnapshot and / or Compact request per group for qe_compact
    (qe_compaction): compact_index / create_index / applied int64 storage of
    the u64 rows (0 = no request; create=False / applied=False leave the row
    out: no snapshot is created, the bound is `committed`), and the outputs
    snap_term (term(i) where a snapshot was created) and result (QE_CP_*)."""

    FIELDS = "compact_index:u64 create_index:u64? applied:u64? snap_term:u64? result:u8"

    def __init__(self, ps, create=True, applied=True):
        dev, i64 = ps.device, torch.int64
        self.compact_index = torch.zeros(ps.G, dtype=i64, device=dev)
        self.create_index = torch.zeros(ps.G, dtype=i64, device=dev) if create else None
        self.applied = torch.zeros(ps.G, dtype=i64, device=dev) if applied else None
        self.snap_term = torch.zeros(ps.G, dtype=i64, device=dev) if create else None
        self.result = torch.zeros(ps.G, dtype=torch.uint8, device=dev)

    def struct(self):
        return _lib.QeCompaction(_ptr(self.compact_index), _ptr(self.create_index),
                                 _ptr(self.applied), _ptr(self.snap_term), _ptr(self.result))


def compact(ps, cp, stats=None):
    """qe_compact: MemoryStorage.CreateSnapshot / Compact on the term runs of
    `ps` (run_first / run_term / run_count, first_index, snap_index), bounded
    by min(applied, committed) -> the Compaction with result / snap_term."""
    p, c = ps.struct(), cp.struct()
    check("qe_compact", _lib.lib().qe_compact(C.byref(p), C.byref(c), _ptr(stats),
                                              _stream(ps.device)))
    return cp


class SnapMsgs(_Rows):
    """One MsgSnap per group for qe_snapshot_step (qe_snap_msgs): type / from_
    u8, term / snap_index / snap_term int64 storage of the u64 fields, the
    ConfState as slot masks in the receiver's numbering (cs_inc, cs_out,
    cs_learner, cs_learners_next), cs_auto_leave u8 and, with ids=True, cs_ids
    [S][stride] (the peer id of each slot)."""

    MASKS = ("cs_inc", "cs_out", "cs_learner", "cs_learners_next")
    FIELDS = ("type:u8 from_:u8 term:u64 snap_index:u64 snap_term:u64 cs_inc:mask cs_out:mask "
              "cs_learner:mask cs_learners_next:mask cs_auto_leave:u8 cs_ids:u64?")

    def __init__(self, ps, ids=False):
        dev, i64, u8 = ps.device, torch.int64, torch.uint8
        self.type = torch.zeros(ps.G, dtype=u8, device=dev)
        self.from_ = torch.zeros(ps.G, dtype=u8, device=dev)
        self.term = torch.zeros(ps.G, dtype=i64, device=dev)
        self.snap_index = torch.zeros(ps.G, dtype=i64, device=dev)
        self.snap_term = torch.zeros(ps.G, dtype=i64, device=dev)
        for k in self.MASKS:
            setattr(self, k, torch.zeros(ps.G, dtype=mask_torch_dtype(ps.S), device=dev))
        self.cs_auto_leave = torch.zeros(ps.G, dtype=u8, device=dev)
        self.cs_ids = torch.zeros(ps.S * ps.stride, dtype=i64, device=dev) if ids else None

    def struct(self):
        return _lib.QeSnapMsgs(*[_ptr(getattr(self, k)) for k in self.ARRAYS])


class SnapOut(_Rows):
    """Outputs of qe_snapshot_step (qe_snap_out): result u8 QE_SR_*,
    resp_index int64 [G] (the MsgAppResp's index where one goes out) and events
    u8 QE_TEV_* [G], written for every group."""

    FIELDS = "result:u8 resp_index:u64 events:u8"

    def __init__(self, ps):
        dev = ps.device
        self.result = torch.zeros(ps.G, dtype=torch.uint8, device=dev)
        self.resp_index = torch.zeros(ps.G, dtype=torch.int64, device=dev)
        self.events = torch.zeros(ps.G, dtype=torch.uint8, device=dev)

    def struct(self):
        return _lib.QeSnapOut(_ptr(self.result), _ptr(self.resp_index), _ptr(self.events))


def snapshot_step(ps, fol, conf, msgs, out=None, stats=None):
    """qe_snapshot_step: one MsgSnap per group through raft.Step's term
    preamble and handleSnapshot / restore on the log rows of `ps` and the
    configuration rows of `conf` (a ConfState; point its inc / out / tracked at
    the tensors of `ps` to restore the rows qe_vote_step and qe_tick read; a row
    set to None is not written) -> SnapOut."""
    if out is None:
        out = SnapOut(ps)
    p, f, c, m, o = ps.struct(), fol.struct(), conf.struct(), msgs.struct(), out.struct()
    check("qe_snapshot_step",
          _lib.lib().qe_snapshot_step(C.byref(p), C.byref(f), C.byref(c), C.byref(m),
                                      C.byref(o), _ptr(stats), _stream(ps.device)))
    return out


class Outbox(_Records):
    """The record arrays of qe_outbox (qe_outbox_out) for up to `capacity`
    messages: group / term / index / log_term / commit int64 storage of the u64
    fields, to / type u8 (QE_OMSG_*), ctx int32, the entries of a MsgApp as
    msg_runs term runs ent_len int32 [E][capacity] / ent_term int64
    [E][capacity], and `count` (int64[1]): the records the masks asked for,
    which may exceed capacity.  The scratch of the call is cached here."""

    FIELDS = ("group:u64 to:u8 type:u8 term:u64 index:u64 log_term:u64 commit:u64 ctx:u32 "
              "ent_len:u32? ent_term:u64? count:u64")
    RUNS = ("ent_len", "ent_term")

    def __init__(self, ps, capacity, msg_runs=_lib.QE_MAX_MSG_RUNS):
        if not 0 <= int(msg_runs) <= _lib.QE_MAX_MSG_RUNS:
            raise ValueError("msg_runs must be 0..QE_MAX_MSG_RUNS")
        self.msg_runs = int(msg_runs)
        self._alloc(ps.device, capacity, self.msg_runs)

    def struct(self):
        return _lib.QeOutboxOut(self.capacity, self.msg_runs, 0, _ptr(self.group), _ptr(self.to),
                                _ptr(self.type), _ptr(self.term), _ptr(self.index),
                                _ptr(self.log_term), _ptr(self.commit), _ptr(self.ctx),
                                _ptr(self.ent_len), _ptr(self.ent_term), _ptr(self.count))


def outbox(ps, term, ob, sent=None, snap=None, index=None, next_before=None, hb_sent=None,
           hb_commit=None, hb_ctx=None, snap_term=None, max_entries=0, stats=None):
    """qe_outbox: the masks of one leader-side call (sent / snap of
    progress_step, propose, become_leader, progress_send, switch_config;
    hb_sent of tick / heartbeat) -> the messages as a dense list in `ob`, in
    (tile, slot, group) order.  `term` is the sender's term row (Follower.term).
    m.Index comes from `index` (PeerMsgs.msg_index) or, for the calls that
    report none, from `next_before` (a clone of ps.next taken before the call;
    ps.next itself after become_leader).  Nothing of `ps` is written."""
    lib = _lib.lib()
    _scratch(ob, ps.device, lib.qe_outbox_scratch_bytes(ps.G))
    p, o = ps.struct(), ob.struct()
    i = _lib.QeOutboxIn(_ptr(sent), _ptr(snap), _ptr(hb_sent), _ptr(index), _ptr(next_before),
                        _ptr(term), _ptr(snap_term), _ptr(hb_commit), _ptr(hb_ctx),
                        int(max_entries), 0)
    check("qe_outbox", lib.qe_outbox(C.byref(p), C.byref(i), C.byref(o), _ptr(ob.scratch),
                                     _ptr(stats), _stream(ps.device)))
    return ob


class Replies(_Records):
    """The record arrays of qe_replies (qe_replies_out) for up to `capacity`
    messages, in the layout an Inbox takes: group / term / index / log_term /
    hint int64 storage of the u64 fields, to / type u8 (QE_IMSG_* or
    QE_RMSG_BAD), ctx int32 and flags u8 (QE_VMF_*; ctx=False / flags=False
    leave the row out: not written), and `count` (int64[1]): the records asked
    for, which may exceed capacity.  The scratch of the call is cached here."""

    FIELDS = ("group:u64 to:u8 type:u8 term:u64 index:u64 log_term:u64 hint:u64 ctx:u32? "
              "flags:u8? count:u64")

    def __init__(self, ps, capacity, ctx=True, flags=True):
        self._alloc(ps.device, capacity,
                    without=(() if ctx else ("ctx",)) + (() if flags else ("flags",)))

    def struct(self):
        return _lib.QeRepliesOut(self.capacity, *[_ptr(getattr(self, k)) for k in self.ARRAYS])


def replies(ps, term, rp, follow=None, snap=None, vote=None, timeout_now=None, f_ctx=None,
            stats=None):
    """qe_replies: what the receiver-side calls sent -> the messages as a dense
    list in `rp`, in (tile, kind, slot, group) order.  follow = (LeaderMsgs,
    FollowerOut), snap = (SnapMsgs, SnapOut) and vote = (VoteMsgs, VoteOut) are
    the message and output objects of follower_step / snapshot_step / vote_step;
    timeout_now is PeerMsgs.timeout_now; f_ctx [G] int32 the contexts the
    heartbeats carried.  `term` is the Follower's term row AFTER those calls.
    Nothing of `ps` is written."""
    lib = _lib.lib()
    _scratch(rp, ps.device, lib.qe_replies_scratch_bytes(ps.G))
    i = _lib.QeRepliesIn(term=_ptr(term), timeout_now=_ptr(timeout_now), f_ctx=_ptr(f_ctx))
    if follow is not None:
        m, o = follow
        i.f_result, i.f_from, i.f_resp_index = _ptr(o.result), _ptr(m.from_), _ptr(o.resp_index)
        i.f_reject_hint, i.f_resp_log_term = _ptr(o.reject_hint), _ptr(o.resp_log_term)
    if snap is not None:
        m, o = snap
        i.s_result, i.s_from, i.s_resp_index = _ptr(o.result), _ptr(m.from_), _ptr(o.resp_index)
    if vote is not None:
        m, o = vote
        i.v_result, i.v_type, i.v_from = _ptr(o.result), _ptr(m.type), _ptr(m.from_)
        i.v_resp_term, i.v_req_log_term = _ptr(o.resp_term), _ptr(o.req_log_term)
        i.v_req_to = _ptr(o.req_to)
    p, o = ps.struct(), rp.struct()
    check("qe_replies", lib.qe_replies(C.byref(p), C.byref(i), C.byref(o), _ptr(rp.scratch),
                                       _ptr(stats), _stream(ps.device)))
    return rp


class ReadyState(_Rows):
    """The resident rows of qe_ready_state [G]: `stable` (unstable.offset - 1),
    `applied`, `snap_pending` (0 = none), prev_term / prev_commit int64 storage
    of the u64 rows, prev_vote / prev_lead / prev_state u8 (rn.prevHardSt and
    rn.prevSoftSt; a slot >= S is None).  Pass the tensor qe_propose /
    qe_compact read as `applied` to share the row."""

    FIELDS = ("stable:u64 applied:u64 snap_pending:u64 prev_term:u64 prev_commit:u64 prev_vote:u8 "
              "prev_lead:u8 prev_state:u8")

    def __init__(self, ps, applied=None):
        dev, i64, u8 = ps.device, torch.int64, torch.uint8
        for k in ("stable", "snap_pending", "prev_term", "prev_commit"):
            setattr(self, k, torch.zeros(ps.G, dtype=i64, device=dev))
        self.applied = applied if applied is not None else torch.zeros(ps.G, dtype=i64, device=dev)
        self.prev_vote = torch.full((ps.G,), 0xFF, dtype=u8, device=dev)
        self.prev_lead = torch.full((ps.G,), 0xFF, dtype=u8, device=dev)
        self.prev_state = torch.zeros(ps.G, dtype=u8, device=dev)

    def reset(self, ps, fol):
        """What NewRawNode does: prev := current, stable = last_index,
        snap_pending = 0.  `applied` is the caller's."""
        self.stable.copy_(ps.last_index)
        self.snap_pending.zero_()
        self.prev_term.copy_(fol.term)
        self.prev_commit.copy_(ps.committed)
        if fol.vote is None:
            self.prev_vote.fill_(0xFF)
        else:
            self.prev_vote.copy_(fol.vote)
        self.prev_lead.copy_(fol.lead)
        self.prev_state.copy_(fol.state)
        return self

    def struct(self):
        return _lib.QeReadyState(*[_ptr(getattr(self, k)) for k in self.ARRAYS])


class Ready(_Records):
    """The record arrays of qe_ready (qe_ready_out) for up to `capacity`
    groups: group / term / commit / ent_first / ent_count / ent_last_term /
    apply_first / apply_count / snap_index int64 storage of the u64 fields,
    vote / lead / state / flags u8 (QE_RD_*), the entries to persist and the
    entries to apply as ent_runs term runs each (ent_len / apply_len int32,
    ent_term / apply_term int64, [E][capacity]), and `count` (int64[1]): the
    groups listed, which may exceed capacity.  The scratch of the call and the
    result row of advance() are cached here."""

    FIELDS = ("group:u64 term:u64 commit:u64 vote:u8 lead:u8 state:u8 flags:u8 ent_first:u64 "
              "ent_count:u64 ent_last_term:u64 apply_first:u64 apply_count:u64 snap_index:u64 "
              "ent_len:u32? ent_term:u64? apply_len:u32? apply_term:u64? count:u64")
    RUNS = ("ent_len", "ent_term", "apply_len", "apply_term")

    def __init__(self, ps, capacity, ent_runs=_lib.QE_MAX_MSG_RUNS):
        if not 0 <= int(ent_runs) <= _lib.QE_MAX_MSG_RUNS:
            raise ValueError("ent_runs must be 0..QE_MAX_MSG_RUNS")
        self.ent_runs = int(ent_runs)
        self._alloc(ps.device, capacity, self.ent_runs)
        self.result = torch.zeros_like(self.flags)

    def struct(self):
        return _lib.QeReadyOut(self.capacity, self.ent_runs, 0,
                               *[_ptr(getattr(self, k)) for k in self.ARRAYS])


def ready_note(ps, rs, follow=None, snap=None):
    """qe_ready_note: keep rs.stable / rs.snap_pending right after a
    follower_step (follow = its FollowerOut) and / or a snapshot_step (snap =
    its SnapOut)."""
    i = _lib.QeReadyNoteIn()
    if follow is not None:
        i.follow_result, i.append_from = _ptr(follow.result), _ptr(follow.append_from)
    if snap is not None:
        i.snap_result, i.snap_resp_index = _ptr(snap.result), _ptr(snap.resp_index)
    p, r = ps.struct(), rs.struct()
    check("qe_ready_note", _lib.lib().qe_ready_note(C.byref(p), C.byref(r), C.byref(i),
                                                    _stream(ps.device)))
    return rs


def ready(ps, fol, rs, rd, pending=None, max_apply=0, stats=None):
    """qe_ready: HasReady + readyWithoutAccept over the batch -> the groups
    that have something to persist or apply as a dense list in `rd`, by
    ascending group.  `pending` [G] u8 marks groups to list whatever their
    state (messages, ReadStates).  Nothing resident is written."""
    lib = _lib.lib()
    _scratch(rd, ps.device, lib.qe_ready_scratch_bytes(ps.G))
    p, f, r, o = ps.struct(), fol.struct(), rs.struct(), rd.struct()
    i = _lib.QeReadyIn(_ptr(pending), int(max_apply), 0)
    check("qe_ready", lib.qe_ready(C.byref(p), C.byref(f), C.byref(r), C.byref(i), C.byref(o),
                                   _ptr(rd.scratch), _ptr(stats), _stream(ps.device)))
    return rd


def advance(ps, rs, rd, fol=None, auto_leave=None, pending_conf_index=None):
    """qe_advance: acceptReady + RawNode.Advance + raft.advance for the records
    of `rd` (a Ready as qe_ready left it, or one the host filled) -> rd.result,
    one QE_ADV_* per record.  With auto_leave / pending_conf_index [G] and
    `fol`, QE_ADV_AUTO_LEAVE marks the leaders that now append the leave-joint
    entry."""
    p, r, o = ps.struct(), rs.struct(), rd.struct()
    f = fol.struct() if fol is not None else None
    opt = _lib.QeAdvanceOpt(_ptr(auto_leave), _ptr(pending_conf_index))
    check("qe_advance", _lib.lib().qe_advance(C.byref(p), C.byref(f) if f is not None else None,
                                              C.byref(r), C.byref(o), C.byref(opt),
                                              _ptr(rd.result), _stream(ps.device)))
    return rd.result


class ReadBook(_Rows):
    """The resident request book of qe_read_book [G][cap] (cap = ps.read_cap,
    or QE_READ_QUEUE when that is 0): `req_index` int64 storage of
    readIndexStatus.index and `req_from` u8 (req.From as a slot, >= S = None)
    of the request with context c of group g, at [g*cap + c % cap]."""

    FIELDS = "req_index:u64 req_from:u8"

    def __init__(self, ps):
        self.cap = max(_lib.QE_READ_QUEUE, ps.read_cap)
        n = ps.G * self.cap
        self.req_index = torch.zeros(n, dtype=torch.int64, device=ps.device)
        self.req_from = torch.full((n,), 0xFF, dtype=torch.uint8, device=ps.device)

    def struct(self):
        return _lib.QeReadBook(_ptr(self.req_index), _ptr(self.req_from))


class ReadStates(_Records):
    """The record arrays of qe_read_states (qe_read_states_out) for up to
    `capacity` records: group / index / key int64 storage of the u64 fields
    (key=False leaves the row out: not written), kind u8 (QE_RS_*), to u8
    (0xFF unless kind is QE_RS_RESP), ctx int32, and `count` (int64[1]): the
    full number of records, which may exceed capacity.  The scratch of the
    call is cached here."""

    FIELDS = "group:u64 kind:u8 to:u8 ctx:u32 index:u64 key:u64? count:u64"

    def __init__(self, ps, capacity, key=True):
        self._alloc(ps.device, capacity, without=() if key else ("key",))

    def struct(self):
        return _lib.QeReadStatesOut(self.capacity,
                                    *[_ptr(getattr(self, k)) for k in self.ARRAYS])


def read_note(ps, book, result, ctx, index, from_=None):
    """qe_read_note: where result[g] == QE_RI_QUEUED, keep index[g] and
    from_[g] (None: every request is local) in `book` under the context
    ctx[g].  result / ctx are the rows read_index returned; `index` is the
    caller's: the row read_index returned, or a round's term_commit_index for
    a postponed read added again."""
    p, b = ps.struct(), book.struct()
    check("qe_read_note", _lib.lib().qe_read_note(C.byref(p), C.byref(b), _ptr(result), _ptr(ctx),
                                                  _ptr(index), _ptr(from_), _stream(ps.device)))
    return book


def read_states(ps, book, rs, msgs=None, ri=None, stats=None):
    """qe_read_states: the answers to ReadIndex requests as a dense list in
    `rs`, by ascending group: the requests the progress_step just run released
    (msgs = its PeerMsgs: read_released, term_commit, term_commit_index) and
    the immediate answers of a read_index call (ri = the tuple it returned,
    optionally extended: (result, ctx, index[, from_[, key]])).  `book` may be
    None without msgs.  Nothing resident is written."""
    lib = _lib.lib()
    _scratch(rs, ps.device, lib.qe_read_states_scratch_bytes(ps.G))
    i = _lib.QeReadStatesIn()
    if msgs is not None:
        i.read_released = _ptr(msgs.read_released)
        i.term_commit, i.term_commit_index = _ptr(msgs.term_commit), _ptr(msgs.term_commit_index)
    if ri is not None:
        ri = tuple(ri) + (None,) * (5 - len(ri))
        i.ri_result, i.ri_index, i.ri_from, i.ri_key = (_ptr(ri[0]), _ptr(ri[2]), _ptr(ri[3]),
                                                        _ptr(ri[4]))
    p, o = ps.struct(), rs.struct()
    b = book.struct() if book is not None else None
    check("qe_read_states", lib.qe_read_states(C.byref(p), C.byref(b) if b is not None else None,
                                               C.byref(i), C.byref(o), _ptr(rs.scratch),
                                               _ptr(stats), _stream(ps.device)))
    return rs


class Inbox(_Rows):
    """The record list of qe_inbox (qe_inbox_in) for up to `capacity` delivered
    messages, and the per-record outputs: group / term / index / log_term /
    commit / hint int64 storage of the u64 fields, from_ / type (QE_IMSG_*) /
    flags (QE_VMF_*) u8, ctx int32, the entries of a MsgApp as msg_runs term
    runs ent_len int32 / ent_term int64 laid out [E][n] for the n records
    loaded; `disposition` u8 (QE_ID_*), `deferred` int32 positions and
    `deferred_count` (int64[1]).  With src=True it also holds the source
    position rows f_src / s_src / v_src [G] and r_src [S][stride] (int32).
    The scratch of the call is cached here."""

    FIELDS = ("group:u64 from_:u8 type:u8 term:u64 index:u64 log_term:u64 commit:u64 hint:u64 "
              "ctx:u32? flags:u8? ent_len:u32? ent_term:u64? disposition:u8 deferred:u32 "
              "deferred_count:u64")
    RECORD = ("group", "from_", "type", "term", "index", "log_term", "commit", "hint", "ctx",
              "flags")

    def __init__(self, ps, capacity, msg_runs=_lib.QE_MAX_MSG_RUNS, ctx=True, flags=True,
                 src=True):
        if not 0 <= int(msg_runs) <= _lib.QE_MAX_MSG_RUNS:
            raise ValueError("msg_runs must be 0..QE_MAX_MSG_RUNS")
        dev, i64, i32, u8 = ps.device, torch.int64, torch.int32, torch.uint8
        self.capacity, self.msg_runs, self.n = int(capacity), int(msg_runs), 0
        c = max(1, self.capacity)
        for k in ("group", "term", "index", "log_term", "commit", "hint"):
            setattr(self, k, torch.zeros(c, dtype=i64, device=dev))
        self.from_ = torch.zeros(c, dtype=u8, device=dev)
        self.type = torch.zeros(c, dtype=u8, device=dev)
        self.ctx = torch.zeros(c, dtype=i32, device=dev) if ctx else None
        self.flags = torch.zeros(c, dtype=u8, device=dev) if flags else None
        e = self.msg_runs * c
        self.ent_len = torch.zeros(e, dtype=i32, device=dev) if e else None
        self.ent_term = torch.zeros(e, dtype=i64, device=dev) if e else None
        self.disposition = torch.zeros(c, dtype=u8, device=dev)
        self.deferred = torch.zeros(c, dtype=i32, device=dev)
        self.deferred_count = torch.zeros(1, dtype=i64, device=dev)
        self.f_src = self.s_src = self.v_src = self.r_src = None
        if src:
            self.f_src = torch.zeros(ps.G, dtype=i32, device=dev)
            self.s_src = torch.zeros(ps.G, dtype=i32, device=dev)
            self.v_src = torch.zeros(ps.G, dtype=i32, device=dev)
            self.r_src = torch.zeros(ps.S * ps.stride, dtype=i32, device=dev)
        self.scratch = None

    def _put(self, n, after, rows, ents):
        """Records after..n-1 from device tensors; the first `after` stay."""
        if not 0 <= after <= self.n or n > self.capacity:
            raise ValueError("the list does not fit the Inbox")
        for k, t in rows.items():
            dst = getattr(self, k)
            if dst is not None:
                dst[after:n].copy_(t)
        E = self.msg_runs
        for k, t in ents.items():
            buf = getattr(self, k)
            if buf is None:
                continue
            new = torch.zeros((E, n), dtype=buf.dtype, device=buf.device)
            new[:, :after] = buf[: E * self.n].view(E, self.n)[:, :after]
            new[:, after:] = t
            buf[: E * n].copy_(new.view(-1))
        self.n = n

    def load_host(self, after=0, **arrays):
        """The list from numpy arrays of the unsigned types (`from` is accepted
        for `from_`): records `after`.. are replaced, the first `after` records
        (a gathered deferred list) stay.  ent_len / ent_term are [E][m] for the
        m records given; a field left out is 0."""
        arrays = {("from_" if k == "from" else k): v for k, v in arrays.items()}
        m = len(arrays["group"])
        n, dev = after + m, self.group.device

        def dev_of(k, shape):
            dt = getattr(self, k).dtype
            if k not in arrays:
                return torch.zeros(shape, dtype=dt, device=dev)
            a = np.ascontiguousarray(arrays[k])
            a = a.view(_SIGNED.get(a.dtype, a.dtype)).reshape(shape)
            return torch.from_numpy(a.copy()).to(dev).to(dt)

        rows = {k: dev_of(k, (m,)) for k in self.RECORD if getattr(self, k) is not None}
        ents = {k: dev_of(k, (self.msg_runs, m)) for k in ("ent_len", "ent_term")
                if getattr(self, k) is not None}
        self._put(n, after, rows, ents)
        return self

    def results(self):
        """-> (disposition[n], the deferred positions, ascending) as numpy."""
        count = int(self.deferred_count.item())
        return (self.disposition[: self.n].cpu().numpy(),
                self.deferred[:count].cpu().numpy().view(np.uint32))

    def gather_deferred(self, out=None):
        """The next pass's list: the DEFERRED records in list order, gathered on
        the device into `out` (default: this Inbox); -> out, with out.n = their
        number.  New arrivals go behind them with load_host(after=out.n, ...)."""
        out = self if out is None else out
        count = int(self.deferred_count.item())
        idx = self.deferred[:count].to(torch.int64)
        rows = {k: getattr(self, k)[idx] for k in self.RECORD
                if getattr(self, k) is not None and getattr(out, k) is not None}
        E = self.msg_runs
        ents = {k: getattr(self, k)[: E * self.n].view(E, self.n)[:, idx]
                for k in ("ent_len", "ent_term") if getattr(self, k) is not None}
        out.n = 0
        out._put(count, 0, rows, ents)
        return out


def inbox(ps, fol, ib, lm, sm, vm, pm, tick_action=None, stats=None):
    """qe_inbox: the list of `ib` routed into the rows of the LeaderMsgs `lm`,
    SnapMsgs `sm`, VoteMsgs `vm` and PeerMsgs `pm` (type / index / reject_hint /
    log_term and, where pm.read_ctx is set, the heartbeat contexts), which then
    go to follower_step, snapshot_step, progress_step and vote_step -- in that
    order: progress_step before vote_step.  `tick_action` is a TickOut's action
    row: its QE_TICK_HUP groups get a QE_VMSG_HUP.  The dispositions and the
    deferred list are left in `ib` (results(), gather_deferred())."""
    if lm.msg_runs != ib.msg_runs:
        raise ValueError("the LeaderMsgs and the Inbox differ in msg_runs")
    lib = _lib.lib()
    _scratch(ib, ps.device, lib.qe_inbox_scratch_bytes(ps.G, ps.S, ib.n),
             grow=lib.qe_inbox_scratch_bytes(ps.G, ps.S, max(1, ib.capacity)))
    p, f = ps.struct(), fol.struct()
    i = _lib.QeInboxIn(ib.n, ib.msg_runs, 0, _ptr(ib.group), _ptr(ib.from_), _ptr(ib.type),
                       _ptr(ib.term), _ptr(ib.index), _ptr(ib.log_term), _ptr(ib.commit),
                       _ptr(ib.hint), _ptr(ib.ctx), _ptr(ib.flags), _ptr(ib.ent_len),
                       _ptr(ib.ent_term), _ptr(tick_action))
    o = _lib.QeInboxOut(
        _ptr(lm.type), _ptr(lm.from_), _ptr(lm.term), _ptr(lm.index), _ptr(lm.log_term),
        _ptr(lm.commit), _ptr(lm.ent_len), _ptr(lm.ent_term),
        _ptr(sm.type), _ptr(sm.from_), _ptr(sm.term), _ptr(sm.snap_index), _ptr(sm.snap_term),
        _ptr(vm.type), _ptr(vm.from_), _ptr(vm.term), _ptr(vm.index), _ptr(vm.log_term),
        _ptr(vm.flags), _ptr(pm.type), _ptr(pm.index), _ptr(pm.reject_hint), _ptr(pm.log_term),
        _ptr(pm.read_ctx), _ptr(ib.f_src), _ptr(ib.s_src), _ptr(ib.v_src), _ptr(ib.r_src),
        _ptr(ib.disposition), _ptr(ib.deferred), _ptr(ib.deferred_count))
    check("qe_inbox", lib.qe_inbox(C.byref(p), C.byref(f), C.byref(i), C.byref(o),
                                   _ptr(ib.scratch), _ptr(stats), _stream(ps.device)))
    return ib


class Peers(_Rows):
    """The host's slot assignment as qe_carry reads it (qe_peers), resident:
    peer_group [S][stride] int64 storage of the global id of the group that is
    the peer in slot s of group g (QE_PEER_NONE: nobody), peer_from [S][stride]
    u8 g's slot in that group's numbering.  A new table has no peer anywhere.
    The scratch of carry() is cached here."""

    FIELDS = "peer_group:u64 peer_from:u8"

    def __init__(self, ps):
        n = ps.S * ps.stride
        self.peer_group = torch.full((n,), -1, dtype=torch.int64, device=ps.device)
        self.peer_from = torch.full((n,), 0xFF, dtype=torch.uint8, device=ps.device)
        self.scratch = None

    @classmethod
    def clusters(cls, ps, N):
        """The static layout of N-node clusters: node i of cluster c is group
        c * N + i of the batch and sits in slot i of every node of c, so the
        peer in slot s < N of g is g - g % N + s and g's slot there is g % N.
        Slots >= N, and the nodes a ragged last cluster lacks, have no peer."""
        g = np.arange(ps.G, dtype=np.uint64)
        pg = np.full((ps.S, ps.stride), _lib.QE_PEER_NONE, np.uint64)
        pf = np.full((ps.S, ps.stride), 0xFF, np.uint8)
        for s in range(min(int(N), ps.S)):
            peer = g - g % np.uint64(N) + np.uint64(s)
            ok = peer < ps.G
            pg[s, :ps.G] = np.where(ok, np.uint64(ps.group_offset) + peer,
                                    np.uint64(_lib.QE_PEER_NONE))
            pf[s, :ps.G] = np.where(ok, g % np.uint64(N), 0xFF).astype(np.uint8)
        return cls(ps).load_host(peer_group=pg, peer_from=pf)

    def struct(self):
        return _lib.QePeers(_ptr(self.peer_group), _ptr(self.peer_from))


class Carried:
    """What carry() leaves: `n` source records read, `count` local records
    appended, `remote_count` records for receivers outside the batch;
    `disposition` u8 [n] (QE_TD_*), `remote` int32 [remote_count] (their source
    positions, ascending) and `src` int32 [count] (the source position of each
    appended record) as device tensors; host() -> (disposition, remote) as
    numpy arrays of the unsigned types."""

    def __init__(self, n, count, remote_count, disposition, remote, src):
        self.n, self.count, self.remote_count = n, count, remote_count
        self.disposition, self.remote, self.src = disposition, remote, src

    def host(self):
        return (self.disposition.cpu().numpy(), self.remote.cpu().numpy().view(np.uint32))


def _mask_arg(a, device):
    """A torch tensor as it is, a numpy array uploaded (bool -> u8)."""
    if a is None or isinstance(a, torch.Tensor):
        return a
    a = np.ascontiguousarray(a)
    a = a.astype(np.uint8) if a.dtype == np.bool_ else a
    return torch.from_numpy(a.view(_SIGNED.get(a.dtype, a.dtype)).copy()).to(device)


def carry(ps, peers, src, ib, after=None, drop=None, cut=None, ignore=0, snap_status=True,
          stats=None):
    """qe_carry: the records an Outbox or a Replies `src` holds, carried to
    their receivers by the Peers table and appended to the Inbox `ib` behind
    its first `after` records (default ib.n), on the device: src's arrays and
    its `count` are read where they are.  drop [>= src's length] u8 / bool
    marks records that are lost, cut [G] mask-typed has bit s of cut[g] set
    where the link g -> slot s is down, `ignore` has bit t set where records of
    type t are lost; with snap_status every MsgSnap carried or lost here is
    reported to its sender (QE_IMSG_SNAP_STATUS / _REJECT behind it).  The
    Inbox keeps its ent rows at pitch n, so the two counts are read once (as
    gather_deferred does).  Raises ValueError, ib.n unchanged, if the records
    do not fit.  -> Carried."""
    lib = _lib.lib()
    after = ib.n if after is None else int(after)
    E_in, E_out = int(getattr(src, "msg_runs", 0)), ib.msg_runs
    if not 0 <= after <= ib.n or E_in > E_out:
        raise ValueError("carry: `after` is past the Inbox's list, or src has more ent runs")
    dev, cap = ps.device, src.capacity
    room = max(0, ib.capacity - after)
    r1 = max(1, room)
    stage = {k: torch.empty(r1, dtype=getattr(ib, k).dtype, device=dev)
             for k in ib.RECORD if getattr(ib, k) is not None}
    ents = {k: torch.empty(E_out * r1, dtype=getattr(ib, k).dtype, device=dev)
            for k in ("ent_len", "ent_term") if getattr(ib, k) is not None}
    o_src = torch.empty(r1, dtype=torch.int32, device=dev)
    disp = torch.empty(max(1, cap), dtype=torch.uint8, device=dev)
    remote = torch.empty(max(1, cap), dtype=torch.int32, device=dev)
    counts = torch.zeros(3, dtype=torch.int64, device=dev)  # local, remote, the source's
    counts[2:3].copy_(src.count)
    drop, cut = _mask_arg(drop, dev), _mask_arg(cut, dev)
    if drop is not None and drop.numel() < cap:  # (the call reads it for i < n <= capacity)
        drop = torch.cat([drop.to(torch.uint8), torch.zeros(cap - drop.numel(), dtype=torch.uint8,
                                                            device=dev)])
    _scratch(peers, dev, lib.qe_carry_scratch_bytes(cap))
    i = _lib.QeCarryIn(cap, _ptr(src.count), E_in, _lib.QE_CARRY_SNAP_STATUS if snap_status else 0,
                       _ptr(src.group), _ptr(src.to), _ptr(src.type), _ptr(src.term),
                       _ptr(src.index), _ptr(src.log_term), _ptr(getattr(src, "commit", None)),
                       _ptr(getattr(src, "hint", None)), _ptr(src.ctx),
                       _ptr(getattr(src, "flags", None)), _ptr(getattr(src, "ent_len", None)),
                       _ptr(getattr(src, "ent_term", None)), _ptr(drop), _ptr(cut), int(ignore), 0)
    o = _lib.QeCarryOut(room, 0, r1, E_out, 0, _ptr(stage["group"]), _ptr(stage["from_"]),
                        _ptr(stage["type"]), _ptr(stage["term"]), _ptr(stage["index"]),
                        _ptr(stage["log_term"]), _ptr(stage["commit"]), _ptr(stage["hint"]),
                        _ptr(stage.get("ctx")), _ptr(stage.get("flags")), _ptr(ents.get("ent_len")),
                        _ptr(ents.get("ent_term")), _ptr(o_src), counts.data_ptr(), _ptr(disp),
                        _ptr(remote), counts.data_ptr() + 8)
    p, pe = ps.struct(), peers.struct()
    check("qe_carry", lib.qe_carry(C.byref(p), C.byref(pe), C.byref(i), C.byref(o),
                                   _ptr(peers.scratch), _ptr(stats), _stream(dev)))
    count, remote_count, n = (int(x) for x in counts.cpu().numpy().view(np.uint64))
    n = min(n, cap)
    if count > room:
        raise ValueError("the carried records do not fit the Inbox")
    ib._put(after + count, after, {k: t[:count] for k, t in stage.items()},
            {k: t.view(E_out, r1)[:, :count] for k, t in ents.items()})
    return Carried(n, count, remote_count, disp[:n], remote[:remote_count], o_src[:count])


class Requests(_Records):
    """The request list of qe_requests (qe_requests_in) for up to
    `list_capacity` records, its per-record outputs and its output list for up
    to `capacity` records (default: list_capacity).  The list rows are q_group /
    q_term / q_index / q_key / q_payload int64 storage of the u64 fields,
    q_type (QE_QMSG_*) / q_from_ (0xFF = None) / q_cc_count u8, q_num_entries
    int32 and, with max_cc > 0, q_cc_pos / q_cc_size int32 and q_cc_leave u8
    laid out [max_cc][n] for the n records loaded.  Per record: `disposition`
    u8 (QE_QD_*) and the deferred positions (`deferred`).  The rows that have
    no home in Proposals / PeerMsgs / VoteMsgs are kept here: ri_request u8,
    ri_key int64 and ri_from u8 [G], and with src=True the source position rows
    p_src / ri_src / v_src [G] and r_src [S][stride] (int32).  The output list
    (records()) is group / term / index / key int64 storage, kind (QE_QO_*) /
    type / to / from_ u8, src int32 and `count` (int64[1]): the full number,
    which may exceed capacity.  The scratch of the call is cached here."""

    FIELDS = "group:u64 kind:u8 type:u8 to:u8 from_:u8 term:u64 index:u64 key:u64 src:u32 count:u64"
    LIST = {"group": "u64", "type": "u8", "from_": "u8", "term": "u64", "index": "u64",
            "key": "u64", "num_entries": "u32", "payload": "u64", "cc_count": "u8"}
    CC = {"cc_pos": "u32", "cc_leave": "u8", "cc_size": "u32"}

    def __init__(self, ps, list_capacity, capacity=None, max_cc=0, src=True):
        if not 0 <= int(max_cc) <= _lib.QE_PROP_MAX_CC:
            raise ValueError("max_cc must be 0..QE_PROP_MAX_CC")
        dev, i64, i32, u8 = ps.device, torch.int64, torch.int32, torch.uint8
        self._alloc(dev, list_capacity if capacity is None else capacity)
        self.list_capacity, self.max_cc, self.n = int(list_capacity), int(max_cc), 0
        c = max(1, self.list_capacity)
        for k, kind in self.LIST.items():
            setattr(self, "q_" + k, torch.zeros(c, dtype=_TORCH[kind], device=dev))
        for k, kind in self.CC.items():
            setattr(self, "q_" + k, torch.zeros(self.max_cc * c, dtype=_TORCH[kind], device=dev)
                    if self.max_cc else None)
        self.ri_request = torch.zeros(ps.G, dtype=u8, device=dev)
        self.ri_key = torch.zeros(ps.G, dtype=i64, device=dev)
        self.ri_from = torch.zeros(ps.G, dtype=u8, device=dev)
        self.disposition = torch.zeros(c, dtype=u8, device=dev)
        self.deferred_pos = torch.zeros(c, dtype=i32, device=dev)
        self.deferred_count = torch.zeros(1, dtype=i64, device=dev)
        self.p_src = self.ri_src = self.v_src = self.r_src = None
        if src:
            self.p_src = torch.zeros(ps.G, dtype=i32, device=dev)
            self.ri_src = torch.zeros(ps.G, dtype=i32, device=dev)
            self.v_src = torch.zeros(ps.G, dtype=i32, device=dev)
            self.r_src = torch.zeros(ps.S * ps.stride, dtype=i32, device=dev)

    def load_host(self, **arrays):
        """The list from numpy arrays of the unsigned types (`from` is accepted
        for `from_`), replacing the one loaded before; cc_pos / cc_leave /
        cc_size are [max_cc][m] for the m records given; a field left out is 0."""
        arrays = {("from_" if k == "from" else k): v for k, v in arrays.items()}
        for k in arrays:
            if k not in self.LIST and k not in self.CC:
                raise KeyError(k)
        m = len(arrays["group"])
        if m > self.list_capacity:
            raise ValueError("the list does not fit the Requests")
        for k in list(self.LIST) + list(self.CC):
            dst = getattr(self, "q_" + k)
            size = m * (self.max_cc if k in self.CC else 1)
            if dst is None or not size:
                continue
            if k not in arrays:
                dst[:size].zero_()
                continue
            a = np.ascontiguousarray(arrays[k])
            a = a.view(_SIGNED.get(a.dtype, a.dtype)).reshape(size)
            dst[:size].copy_(torch.from_numpy(a.copy()).to(dst.device).to(dst.dtype))
        self.n = m
        return self

    @property
    def deferred(self):
        """The positions of the DEFERRED records, ascending (numpy uint32)."""
        count = int(self.deferred_count.item())
        return self.deferred_pos[:count].cpu().numpy().view(np.uint32)

    def dispositions(self):
        return self.disposition[: self.n].cpu().numpy()


def requests(ps, fol, rq, props, pm, vm, stats=None, no_forward=False):
    """qe_requests: the request list of `rq` handled as raft.Step would on each
    record's receiver.  The leader-side rows go into the Proposals `props`
    (num_entries, payload and the conf-change rows), rq.ri_request / ri_key /
    ri_from (for read_index, read_note and read_states), pm.type of the
    PeerMsgs `pm` (QE_MSG_TRANSFER_LEADER) and the VoteMsgs `vm` (a higher
    term); the steps then run in the order propose, read_index, read_note,
    progress_step, vote_step, read_states.  no_forward is
    Config.DisableProposalForwarding.  The dispositions, the deferred
    positions and the output list are left in `rq`."""
    if props.max_cc != rq.max_cc:
        raise ValueError("the Proposals and the Requests differ in max_cc")
    lib = _lib.lib()
    _scratch(rq, ps.device, lib.qe_requests_scratch_bytes(ps.G, rq.n),
             grow=lib.qe_requests_scratch_bytes(ps.G, max(1, rq.list_capacity)))
    p, f = ps.struct(), fol.struct()
    i = _lib.QeRequestsIn(
        rq.n, rq.max_cc, _lib.QE_REQ_NO_FORWARD if no_forward else 0, _ptr(rq.q_group),
        _ptr(rq.q_type), _ptr(rq.q_from_), _ptr(rq.q_term), _ptr(rq.q_index), _ptr(rq.q_key),
        _ptr(rq.q_num_entries), _ptr(rq.q_payload), _ptr(rq.q_cc_count), _ptr(rq.q_cc_pos),
        _ptr(rq.q_cc_leave), _ptr(rq.q_cc_size), 0)
    o = _lib.QeRequestsOut(
        _ptr(props.num_entries), _ptr(props.payload), _ptr(props.cc_count), _ptr(props.cc_pos),
        _ptr(props.cc_leave), _ptr(props.cc_size), props.G,
        _ptr(rq.ri_request), _ptr(rq.ri_key), _ptr(rq.ri_from),
        _ptr(vm.type), _ptr(vm.from_), _ptr(vm.term), _ptr(vm.index), _ptr(vm.log_term),
        _ptr(vm.flags), _ptr(pm.type), _ptr(rq.p_src), _ptr(rq.ri_src), _ptr(rq.v_src),
        _ptr(rq.r_src), _ptr(rq.disposition), _ptr(rq.deferred_pos), _ptr(rq.deferred_count),
        rq.capacity, *[_ptr(getattr(rq, k)) for k in rq.ARRAYS])
    check("qe_requests", lib.qe_requests(C.byref(p), C.byref(f), C.byref(i), C.byref(o),
                                         _ptr(rq.scratch), _ptr(stats), _stream(ps.device)))
    return rq


class Proposals:
    """One MsgProp per group for qe_propose (qe_proposals, ABI 6):
    num_entries [G] (0 = none), payload [G] (sum of the non-conf-change
    entries' PayloadSize), up to max_cc conf-change entries per proposal
    ([max_cc][G]: position, leave-joint flag, size), applied /
    pending_conf_index / uncommitted_size [G], and the outputs result,
    cc_refused, sent, snap [G]."""

    def __init__(self, ps, max_cc=0, max_uncommitted=0, track_uncommitted=True, flags=0):
        G, dev = ps.G, ps.device
        self.G, self.max_cc, self.max_uncommitted = G, int(max_cc), int(max_uncommitted)
        self.flags = int(flags)  # QE_PROP_APPEND_ONLY: appendEntry alone
        i64 = torch.int64
        self.num_entries = torch.zeros(G, dtype=torch.int32, device=dev)
        self.payload = torch.zeros(G, dtype=i64, device=dev)
        c = max(1, self.max_cc)
        self.cc_count = torch.zeros(G, dtype=torch.uint8, device=dev)
        self.cc_pos = torch.zeros(c * G, dtype=torch.int32, device=dev)
        self.cc_leave = torch.zeros(c * G, dtype=torch.uint8, device=dev)
        self.cc_size = torch.zeros(c * G, dtype=torch.int32, device=dev)
        self.applied = torch.zeros(G, dtype=i64, device=dev)
        self.pending_conf_index = torch.zeros(G, dtype=i64, device=dev)
        self.uncommitted_size = torch.zeros(G, dtype=i64, device=dev) if track_uncommitted else None
        self.result = torch.zeros(G, dtype=torch.uint8, device=dev)
        self.cc_refused = torch.zeros(G, dtype=torch.uint8, device=dev)
        md = mask_torch_dtype(ps.S)
        self.sent = torch.zeros(G, dtype=md, device=dev)
        self.snap = torch.zeros(G, dtype=md, device=dev)
        self.bytes_requested = None

    def struct(self):
        cc = self.max_cc > 0
        return _lib.QeProposals(
            _ptr(self.num_entries), _ptr(self.payload), self.max_cc, self.flags, self.G,
            _ptr(self.cc_count) if cc else None, _ptr(self.cc_pos) if cc else None,
            _ptr(self.cc_leave) if cc else None, _ptr(self.cc_size) if cc else None,
            _ptr(self.applied), _ptr(self.pending_conf_index), _ptr(self.uncommitted_size),
            self.max_uncommitted, _ptr(self.result), _ptr(self.cc_refused), _ptr(self.sent),
            _ptr(self.snap), _ptr(self.bytes_requested))


def propose(ps, props, stats=None):
    """qe_propose: stepLeader's MsgProp + appendEntry + bcastAppend
    (raft/raft.go:1019-1076, :621-642, :515-522) for every group with
    num_entries > 0; advances ps.last_index."""
    p, q = ps.struct(), props.struct()
    check("qe_propose", _lib.lib().qe_propose(C.byref(p), C.byref(q), _ptr(stats),
                                               _stream(ps.device)))


def propose_bytes_requested(ps, props):
    """The algorithmic bytes of one qe_propose launch (instrumented variant,
    field granularity); mutates the state like propose."""
    acct = torch.zeros(1, dtype=torch.int64, device=ps.device)
    props.bytes_requested = acct
    try:
        propose(ps, props)
    finally:
        props.bytes_requested = None
    return int(acct.item())


class Switch:
    """One qe_switch_config call's per-group flags and outputs (qe_switch,
    ABI 7): switched [G] (None = every group), result [G] (QE_SW_*, bit
    QE_SW_TRANSFER_ABORTED), sent / snap masks [G]."""

    def __init__(self, ps, switched=None):
        G, dev = ps.G, ps.device
        self.switched = switched
        self.result = torch.zeros(G, dtype=torch.uint8, device=dev)
        md = mask_torch_dtype(ps.S)
        self.sent = torch.zeros(G, dtype=md, device=dev)
        self.snap = torch.zeros(G, dtype=md, device=dev)
        self.bytes_requested = None

    def struct(self):
        return _lib.QeSwitch(_ptr(self.switched), _ptr(self.result), _ptr(self.sent),
                             _ptr(self.snap), _ptr(self.bytes_requested))


def switch_config(ps, sw, stats=None):
    """qe_switch_config: raft.switchToConfig (raft/raft.go:1651-1700) on every
    group with sw.switched[g], the new configuration being ps's inc / out /
    tracked masks: maybeCommit under it, then bcastAppend or the probe of
    every peer, and abortLeaderTransfer for a transferee no longer a voter."""
    p, q = ps.struct(), sw.struct()
    check("qe_switch_config", _lib.lib().qe_switch_config(C.byref(p), C.byref(q), _ptr(stats),
                                                           _stream(ps.device)))
    return sw


def switch_bytes_requested(ps, sw):
    """The algorithmic bytes of one qe_switch_config launch (instrumented
    variant, field granularity); mutates the state like switch_config."""
    acct = torch.zeros(1, dtype=torch.int64, device=ps.device)
    sw.bytes_requested = acct
    try:
        switch_config(ps, sw)
    finally:
        sw.bytes_requested = None
    return int(acct.item())


class Leader:
    """One qe_become_leader call's per-group inputs and outputs (qe_leader,
    ABI 7): elected [G] (None = every group), term [G], pending_conf_index /
    uncommitted_size [G] outputs, result [G] (QE_BL_*), sent / snap masks."""

    def __init__(self, ps, elected=None, bcast=True):
        G, dev = ps.G, ps.device
        self.elected = elected
        self.term = torch.zeros(G, dtype=torch.int64, device=dev)
        self.flags = _lib.QE_BL_BCAST if bcast else 0
        self.pending_conf_index = torch.zeros(G, dtype=torch.int64, device=dev)
        self.uncommitted_size = torch.zeros(G, dtype=torch.int64, device=dev)
        self.result = torch.zeros(G, dtype=torch.uint8, device=dev)
        md = mask_torch_dtype(ps.S)
        self.sent = torch.zeros(G, dtype=md, device=dev)
        self.snap = torch.zeros(G, dtype=md, device=dev)

    def struct(self):
        return _lib.QeLeader(_ptr(self.elected), _ptr(self.term), self.flags, 0,
                             _ptr(self.pending_conf_index), _ptr(self.uncommitted_size),
                             _ptr(self.result), _ptr(self.sent), _ptr(self.snap))


def become_leader(ps, ld, stats=None):
    """qe_become_leader: raft.becomeLeader (raft/raft.go:724-759, reset
    :590-613) on every group with ld.elected[g] -- every Progress reset, the
    log model enters ld.term[g], the empty entry appended and (bcast)
    stepCandidate's bcastAppend."""
    p, q = ps.struct(), ld.struct()
    check("qe_become_leader", _lib.lib().qe_become_leader(C.byref(p), C.byref(q), _ptr(stats),
                                                           _stream(ps.device)))
    return ld


class ConfState:
    """Device-resident tracker.Config + ProgressMap key set of G groups in
    slot form (qe_conf): slot_ids ID-major [S][G], slot masks for Voters[0],
    Voters[1], Learners, LearnersNext, Progress.IsLearner and tracked slots,
    and AutoLeave."""

    MASKS = ("inc", "out", "learner", "learners_next", "is_learner", "tracked")

    def __init__(self, G, S, device="cuda"):
        if not 1 <= S <= _lib.QE_MAX_SLOTS:
            raise ValueError("bad num_slots")
        self.G, self.S, self.device = int(G), int(S), torch.device(device)
        md = mask_torch_dtype(S)
        self.slot_ids = torch.zeros(self.G * self.S, dtype=torch.int64, device=self.device)
        for k in self.MASKS:
            setattr(self, k, torch.zeros(self.G, dtype=md, device=self.device))
        self.auto_leave = torch.zeros(self.G, dtype=torch.uint8, device=self.device)

    def struct(self):
        return _lib.QeConf(self.G, self.S, 0, _ptr(self.slot_ids), _ptr(self.inc), _ptr(self.out),
                           _ptr(self.learner), _ptr(self.learners_next), _ptr(self.is_learner),
                           _ptr(self.tracked), _ptr(self.auto_leave))

    def host(self):
        md = mask_np_dtype(self.S)
        out = {"slot_ids": self.slot_ids.cpu().numpy().view(np.uint64).reshape(self.S, self.G).T,
               "auto_leave": self.auto_leave.cpu().numpy()}
        for k in self.MASKS:
            out[k] = getattr(self, k).cpu().numpy().view(md)
        return out


class ConfChanges:
    """One configuration-change operation per group (qe_conf_changes):
    op [G], count [G], type/node_id [C][stride], last_index [G]; result and
    new_progress are outputs."""

    def __init__(self, G, S, C_max, device="cuda"):
        self.G, self.C = int(G), int(C_max)
        self.stride = max(1, self.G)
        dev = torch.device(device)
        self.op = torch.zeros(self.G, dtype=torch.uint8, device=dev)
        self.count = torch.zeros(self.G, dtype=torch.uint8, device=dev)
        self.type = torch.zeros(max(1, self.C) * self.stride, dtype=torch.uint8, device=dev)
        self.node_id = torch.zeros(max(1, self.C) * self.stride, dtype=torch.int64, device=dev)
        self.last_index = torch.zeros(self.G, dtype=torch.int64, device=dev)
        self.result = torch.zeros(self.G, dtype=torch.uint8, device=dev)
        self.new_progress = torch.zeros(self.G, dtype=mask_torch_dtype(S), device=dev)

    def struct(self):
        return _lib.QeConfChanges(self.C, 0, self.stride, _ptr(self.op), _ptr(self.count),
                                  _ptr(self.type), _ptr(self.node_id), _ptr(self.last_index),
                                  _ptr(self.result), _ptr(self.new_progress))


def confchange(cs, ch, ps=None):
    """Changer.Simple / EnterJoint / LeaveJoint per group on the GPU
    (qe_confchange, raft/confchange/confchange.go:49-274)."""
    c, x = cs.struct(), ch.struct()
    p = C.byref(ps.struct()) if ps is not None else None
    check("qe_confchange", _lib.lib().qe_confchange(C.byref(c), C.byref(x), p,
                                                     _stream(cs.device)))


class ApplyConf(_Records):
    """The record list of qe_apply_conf (qe_apply_conf_in) for up to `capacity`
    committed conf-change entries and its per-record outputs
    (qe_apply_conf_out).  The list rows are q_group int64 storage of the u64
    field, q_transition (QE_AC_AUTO ...) / q_num_changes u8 and, laid out
    [max_changes][capacity], q_type u8 (QE_CC_ADD_NODE ...), q_node_id int64 and
    with slots=True q_slot u8 (QE_AC_ANY_SLOT = the lowest untracked slot).
    Per record: result (QE_AC_*), cc_result (QE_CC_*), sw_result (QE_SW_*) u8,
    the ConfState after the record as slot masks inc / out / learner /
    learners_next / tracked / new_progress and auto_leave u8, and with ids=True
    the tracked slots' ids [S][capacity].  `count` (int64[1]) is the device
    count qe_apply_conf reads with device_count=True; load_host sets it.  The
    scratch of the call is cached here."""

    FIELDS = ("result:u8 cc_result:u8 sw_result:u8 inc:mask out:mask learner:mask "
              "learners_next:mask tracked:mask new_progress:mask auto_leave:u8 ids:u64? count:u64")
    RUNS = ("ids",)
    LIST = {"group": "u64", "transition": "u8", "num_changes": "u8"}
    CHANGES = {"type": "u8", "node_id": "u64", "slot": "u8"}

    def __init__(self, ps, capacity, max_changes=1, slots=True, ids=True, device_count=False):
        if not 0 <= int(max_changes) <= 255:
            raise ValueError("max_changes must be 0..255")
        dev = ps.device
        self.S, self.max_changes, self.n = ps.S, int(max_changes), 0
        self.device_count = bool(device_count)
        self.capacity = int(capacity)
        c = max(1, self.capacity)
        md = mask_torch_dtype(ps.S)
        for k in self.ARRAYS:
            kind = self.KIND[k]
            size = 1 if k == "count" else ps.S * c if k == "ids" else c
            t = None if (k == "ids" and not ids) else torch.zeros(
                size, dtype=md if kind == "mask" else _TORCH[kind], device=dev)
            setattr(self, k, t)
        for k, kind in self.LIST.items():
            setattr(self, "q_" + k, torch.zeros(c, dtype=_TORCH[kind], device=dev))
        for k, kind in self.CHANGES.items():
            setattr(self, "q_" + k, None if (k == "slot" and not slots) else
                    torch.zeros(max(1, self.max_changes) * c, dtype=_TORCH[kind], device=dev))
        self.scratch = None

    def load_host(self, **arrays):
        """The list from numpy arrays of the unsigned types, replacing the one
        loaded before: group / transition / num_changes [m], type / node_id /
        slot [max_changes][m] for the m records given.  A field left out is 0
        (slot: QE_AC_ANY_SLOT).  m may exceed the capacity: the rows then hold
        the first `capacity` records and qe_apply_conf sees n = m."""
        for k in arrays:
            if k not in self.LIST and k not in self.CHANGES:
                raise KeyError(k)
        m = len(arrays["group"])
        keep, cap = min(m, self.capacity), max(1, self.capacity)
        for k in list(self.LIST) + list(self.CHANGES):
            dst = getattr(self, "q_" + k)
            if dst is None:
                continue
            rows = self.max_changes if k in self.CHANGES else 1
            if not rows:
                continue
            dst.fill_(_lib.QE_AC_ANY_SLOT if k == "slot" else 0)
            if k not in arrays or not keep:
                continue
            a = np.ascontiguousarray(arrays[k])
            a = a.view(_SIGNED.get(a.dtype, a.dtype)).reshape(rows, m)[:, :keep]
            dst.view(-1, cap)[:rows, :keep].copy_(torch.from_numpy(a.copy()).to(dst.device))
        self.n = m
        self.count.fill_(m)
        return self

    def records(self):
        """-> (n, the per-record outputs cut to min(n, capacity) as numpy
        arrays; ids as [S][n], None when left out)."""
        n, cap = min(self.n, self.capacity), max(1, self.capacity)
        out = {}
        for k, a in self.host().items():
            if k == "count":
                continue
            out[k] = None if a is None else a.reshape(-1, cap)[:, :n] if k in self.RUNS else a[:n]
        return self.n, out

    def results(self):
        """-> (result, cc_result, sw_result) of the min(n, capacity) records."""
        n = min(self.n, self.capacity)
        return tuple(getattr(self, k)[:n].cpu().numpy() for k in ("result", "cc_result", "sw_result"))

    def struct_in(self):
        return _lib.QeApplyConfIn(
            self.capacity, self.n, _ptr(self.count) if self.device_count else None,
            self.max_changes, 0, _ptr(self.q_group), _ptr(self.q_transition),
            _ptr(self.q_num_changes), _ptr(self.q_type), _ptr(self.q_node_id), _ptr(self.q_slot))

    def struct_out(self):
        return _lib.QeApplyConfOut(*[_ptr(getattr(self, k)) for k in self.ARRAYS if k != "count"])


def apply_conf(ps, fol, conf, ac, sw=None):
    """qe_apply_conf: the committed conf-change entries listed in `ac` applied
    as RawNode.ApplyConfChange does, on every role: the ConfChangeV2 decoded
    and the Changer run on `conf` (and on ps's inc / out / tracked where those
    are other tensors), initProgress for the created slots, and for the groups
    that lead switchToConfig's leader half (qe_switch_config's kernel) on a
    `switched` row the call keeps in its scratch.  With a Switch `sw` its
    result / sent / snap rows are filled for qe_outbox.  The per-record results
    and ConfStates are left in `ac`."""
    lib = _lib.lib()
    _scratch(ac, ps.device, lib.qe_apply_conf_scratch_bytes(ps.G) + 16)
    base = ac.scratch.data_ptr()
    p, f, c, i, o = ps.struct(), fol.struct(), conf.struct(), ac.struct_in(), ac.struct_out()
    q = C.byref(sw.struct()) if sw is not None else None
    check("qe_apply_conf", lib.qe_apply_conf(C.byref(p), C.byref(f), C.byref(c), C.byref(i),
                                             C.byref(o), q, (base + 15) & ~15,
                                             _stream(ps.device)))
    return ac
