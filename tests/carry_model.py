"""qe_carry restated in numpy (include/etcd_quorum.h states the rules): a list
of sent records (`group` the sender, `to` a slot of the sender) -> a disposition
per record, the local list in qe_inbox's layout (`group` the receiver, `from`
the sender's slot there) with the MsgSnapStatus records of duty H11, the remote
positions and the statistics.  Beside it the reference's in-process network
(raft/raft_test.go:4633-4778) restated over message dicts: `Network.filter`
and the addressing of `send`.  Imports no torch.

carry() takes the source as a dict of numpy arrays of `capacity` records
(group, to, type, term, index, log_term; commit, hint, ctx, mflags optional;
ent_len / ent_term [E_in][capacity]) with "count", and returns the WHOLE local
list; place() writes it into output arrays as the call does (base, capacity,
ent pitch), so a test compares arrays whole, tails included."""
from types import SimpleNamespace

import numpy as np

from tests.inbox_model import record_hashes

APP, SNAP, HEARTBEAT = 1, 2, 3
SNAP_STATUS, SNAP_STATUS_REJECT, HUP = 7, 8, 16
CARRIABLE = tuple(range(1, 7)) + tuple(range(10, 16))
CARRY_TYPES = sum(1 << t for t in CARRIABLE)
LOCAL, REMOTE, LOST, BAD = 1, 2, 3, 255
PEER_NONE = 0xFFFFFFFFFFFFFFFF
SALT = 0x8CB92BA72F3D8DD7
STAT_GROUPS, STAT_BAD, STAT_LOCAL, STAT_LOST, STAT_REMOTE, STAT_SNAP_STATUS = 0, 1, 4, 5, 6, 9
STAT_VIOLATIONS, STAT_CHECKSUM = 14, 15
U64 = ("group", "term", "index", "log_term", "commit", "hint")
FIELDS = {"group": np.uint64, "from": np.uint8, "type": np.uint8, "term": np.uint64,
          "index": np.uint64, "log_term": np.uint64, "commit": np.uint64, "hint": np.uint64,
          "ctx": np.uint32, "mflags": np.uint8, "src": np.uint32}
ENTS = {"ent_len": np.uint32, "ent_term": np.uint64}


def carry(st, peer_group, peer_from, src, drop=None, cut=None, ignore=0, snap_status=True,
          msg_runs_out=None):
    """-> SimpleNamespace(n, disposition [n], count, local {field: [count]; ent_len / ent_term
    [E_out][count]}, remote [remote_count], stats [16])."""
    G, S, stride = st.num_groups, st.num_slots, st.stride
    goff = np.uint64(st.group_offset)
    cap = len(src["group"])
    n = min(int(src["count"]), cap)
    E_in = 0 if src.get("ent_len") is None else len(src["ent_len"])
    E_out = E_in if msg_runs_out is None else msg_runs_out
    assert E_in <= E_out and not ignore & ~CARRY_TYPES
    gid = np.asarray(src["group"][:n], np.uint64)
    to = np.asarray(src["to"][:n]).astype(np.int64)
    typ = np.asarray(src["type"][:n]).astype(np.int64)
    with np.errstate(over="ignore"):
        g = gid - goff
    # rule 1
    typed = np.isin(typ, CARRIABLE)
    inb = typed & (g < np.uint64(G)) & (to < S)
    k = np.where(inb, to * stride + g.astype(np.int64), 0)
    pg = np.where(inb, np.asarray(peer_group, np.uint64).reshape(-1)[k], np.uint64(PEER_NONE))
    pf = np.where(inb, np.asarray(peer_from, np.uint8).reshape(-1)[k], 0xFF).astype(np.int64)
    with np.errstate(over="ignore"):
        here = (pg - goff) < np.uint64(G)
    ok = inb & (pg != np.uint64(PEER_NONE)) & ~(here & (pf >= S))
    # rule 2: only the sender's link bit is read
    lost = ((ignore >> np.where(typed, typ, 0)) & 1) != 0
    if drop is not None:
        lost |= np.asarray(drop[:n]) != 0
    if cut is not None:
        bits = np.asarray(cut).astype(np.int64)[np.where(inb, g.astype(np.int64), 0)]
        lost |= ((bits >> np.where(inb, to, 0)) & 1) != 0
    lost &= ok
    # rules 3-5
    remote, local = ok & ~lost & ~here, ok & ~lost & here
    disp = np.where(~ok, BAD, np.where(lost, LOST, np.where(here, LOCAL, REMOTE))).astype(np.uint8)
    snap = (typ == SNAP) & bool(snap_status)
    kc = np.where(local, 1 + snap, np.where(lost & snap, 1, 0)).astype(np.int64)
    start, count = np.cumsum(kc) - kc, int(kc.sum())
    out = {f: np.zeros(count, t) for f, t in FIELDS.items()}
    out.update({f: np.zeros((E_out, count), t) for f, t in ENTS.items()})
    i1, i2 = np.flatnonzero(local), np.flatnonzero(lost & snap)
    p1 = start[i1]
    out["group"][p1], out["from"][p1], out["type"][p1] = pg[i1], pf[i1], typ[i1]
    for f in ("term", "index", "log_term", "commit", "hint", "ctx", "mflags"):
        if src.get(f) is not None:
            out[f][p1] = np.asarray(src[f])[:n][i1]
    for f in ENTS:
        for j in range(E_in):
            out[f][j, p1] = np.asarray(src[f][j])[:n][i1]
    out["src"][p1] = i1
    # the status records: term 0 and every other field 0
    for idx, pos, t in ((i2, start[i2], SNAP_STATUS_REJECT),
                        (np.flatnonzero(kc == 2), start[kc == 2] + 1, SNAP_STATUS)):
        out["group"][pos], out["from"][pos], out["type"][pos], out["src"][pos] = \
            gid[idx], to[idx], t, idx
    stats = np.zeros(16, np.uint64)
    stats[STAT_GROUPS] = count
    stats[STAT_LOCAL], stats[STAT_REMOTE], stats[STAT_LOST] = local.sum(), remote.sum(), lost.sum()
    stats[STAT_BAD] = stats[STAT_VIOLATIONS] = (~ok).sum()
    stats[STAT_SNAP_STATUS] = (snap & (local | lost)).sum()
    with np.errstate(over="ignore"):
        stats[STAT_CHECKSUM] = record_hashes(gid, disp, typ, to, SALT).sum(dtype=np.uint64)
    return SimpleNamespace(n=n, disposition=disp, count=count, local=out, msg_runs=E_out,
                           remote=np.flatnonzero(remote).astype(np.uint32), stats=stats)


def place(res, arrays, base, capacity, ent_pitch):
    """The local list of `res` into `arrays` (flat, prefilled) as the call writes it: record k
    at base + k, ent rows at [j * ent_pitch + base + k], nothing at or past capacity."""
    m = max(0, min(base + res.count, capacity) - base)
    for f, a in arrays.items():
        if a is None:
            continue
        if f in ENTS:
            for j in range(res.msg_runs):
                a[j * ent_pitch + base: j * ent_pitch + base + m] = res.local[f][j, :m]
        else:
            a[base: base + m] = res.local[f][:m]
    return arrays


class Network:
    """The reference's test network over message dicts (type, from, to = node ids, ...):
    ignorem, dropm by directed link, msgHook; filter() as raft_test.go:4750-4774 decides,
    `rand` standing for rand.Float64."""

    def __init__(self, rand, msg_hook=None):
        self.dropm, self.ignorem, self.rand, self.msg_hook = {}, set(), rand, msg_hook

    def drop(self, frm, to, perc):
        self.dropm[frm, to] = perc

    def cut(self, one, other):
        self.drop(one, other, 2.0)
        self.drop(other, one, 2.0)

    def isolate(self, node, nodes):
        for other in nodes:
            if other != node:
                self.drop(node, other, 1.0)
                self.drop(other, node, 1.0)

    def ignore(self, t):
        self.ignorem.add(t)

    def filter(self, msgs):
        kept = []
        for m in msgs:
            if m["type"] in self.ignorem:
                continue
            if m["type"] == HUP:
                raise RuntimeError("unexpected msgHup")  # hups never go over the network
            if self.rand() < self.dropm.get((m["from"], m["to"]), 0.0):
                continue
            if self.msg_hook is not None and not self.msg_hook(m):
                continue
            kept.append(m)
        return kept


def deliver(slot_ids, group_of, msgs):
    """send's addressing: m.To names the receiver (group_of[id]); the sender's slot in the
    receiver's numbering is where the receiver's slot table (slot_ids[receiver group]) holds
    m.From -> the records (group, from, ...) in order."""
    out = []
    for m in msgs:
        r = group_of[m["to"]]
        out.append(dict(m, group=r, **{"from": list(slot_ids[r]).index(m["from"])}))
    return out


# ---- the cases the model's test and the GPU test share ----
LENGTHS = (0, 1, 63, 64, 65, 4096 + 65, 2 * 4096 + 1)
BAD_TYPES = (0, 7, 8, 9, 16, 17, 255)


def tables(rng, G, S, stride, goff, N=3, foreign=True):
    """A peer table of N-node clusters (node i of cluster c is group c * N + i) whose slots
    are permuted per node -> (peer_group, peer_from [S][stride], slot_ids [G][S] node ids,
    0 = none; a node's id is its global group id + 1).  With `foreign`, some peers are
    replaced by ids outside the batch, some by QE_PEER_NONE, and a few in-batch entries get
    a peer_from that is no slot."""
    assert G % N == 0 and S >= N
    slot_of = np.full((G, G), -1, np.int64)   # slot_of[g][h]: h's slot in g's numbering
    peer = np.full((S, G), -1, np.int64)
    for g in range(G):
        slots = rng.permutation(S)[:N]
        for i in range(N):
            h = g - g % N + i
            slot_of[g, h], peer[slots[i], g] = slots[i], h
    pg = np.full((S, stride), PEER_NONE, np.uint64)
    pf = np.full((S, stride), 0xFF, np.uint8)
    ids = np.zeros((G, S), np.uint64)
    for s in range(S):
        for g in range(G):
            h = peer[s, g]
            if h >= 0:
                pg[s, g], pf[s, g], ids[g, s] = goff + h, slot_of[h, g], goff + h + 1
    if foreign:
        r = rng.random((S, stride))
        has = pg != np.uint64(PEER_NONE)
        away = goff + G + rng.integers(0, 1000, (S, stride)).astype(np.uint64)
        if goff:
            away = np.where(rng.random((S, stride)) < 0.5, np.uint64(goff) - np.uint64(5), away)
        pg = np.where(has & (r < 0.15), away.astype(np.uint64), pg)
        pf = np.where(has & (r < 0.15), rng.integers(0, 256, (S, stride)), pf).astype(np.uint8)
        pg = np.where(has & (r >= 0.15) & (r < 0.2), np.uint64(PEER_NONE), pg)
        pf = np.where(has & (r >= 0.2) & (r < 0.24), S + rng.integers(0, 200, (S, stride)) % (256 - S),
                      pf).astype(np.uint8)
    return pg, pf, ids


def big(rng, size):
    """u64 values, half of them above 2^63."""
    v = rng.integers(0, 1 << 62, size).astype(np.uint64)
    return np.where(rng.random(size) < 0.5, v | np.uint64(1 << 63), v)


def source(rng, st, peer_group, cap, count, form, E_in):
    """A source list of `cap` generated records ("count" may be below or above cap): mostly
    carriable types to slots of the batch, a quarter MsgSnap, some of each BAD cause."""
    G, S, goff = st.num_groups, st.num_slots, st.group_offset
    r = rng.random(cap)
    group = np.uint64(goff) + rng.integers(0, G, cap).astype(np.uint64)
    outside = np.uint64(goff + G) + rng.integers(0, 50, cap).astype(np.uint64)
    if goff:
        outside = np.where(rng.random(cap) < 0.5, np.uint64(goff - 1), outside)
    group = np.where(r < 0.03, outside, group).astype(np.uint64)
    # `to`: mostly a slot that has a peer, else any slot, a few no slot at all
    occupied = np.asarray(peer_group)[:, :G] != np.uint64(PEER_NONE)
    order, have = np.argsort(~occupied, axis=0, kind="stable"), occupied.sum(axis=0)
    gl = rng.integers(0, G, cap)
    group = np.where(r < 0.03, group, np.uint64(goff) + gl.astype(np.uint64))
    peered = order[rng.integers(0, 1 << 30, cap) % np.maximum(have[gl], 1), gl]
    to = np.where(r < 0.06, rng.integers(S, 256, cap),
                  np.where((r < 0.85) & (have[gl] > 0), peered, rng.integers(0, S, cap)))
    to = to.astype(np.uint8)
    t = rng.random(cap)
    typ = np.where(t < 0.25, SNAP, np.where(t < 0.9, rng.choice(CARRIABLE, cap),
                                            rng.choice(BAD_TYPES, cap))).astype(np.uint8)
    src = dict(count=count, group=group, to=to, type=typ, term=big(rng, cap), index=big(rng, cap),
               log_term=big(rng, cap), ctx=rng.integers(0, 1 << 32, cap).astype(np.uint32))
    if form == "outbox":
        src["commit"] = big(rng, cap)
        if E_in:
            src["ent_len"] = rng.integers(0, 1 << 32, (E_in, cap)).astype(np.uint32)
            src["ent_term"] = big(rng, (E_in, cap))
    else:
        src["hint"] = big(rng, cap)
        src["mflags"] = rng.integers(0, 256, cap).astype(np.uint8)
    return src


def make_case(name, seed, n, G, S, E, goff, form, stats, cap=None, count=None, snap_status=True):
    rng = np.random.default_rng(seed)
    E_in, E_out = E if form == "outbox" else (0, 4 if E[1] == 4 else 0)  # (a replies list has no runs)
    st = SimpleNamespace(num_groups=G, group_offset=goff, num_slots=S, stride=G + 3)
    pg, pf, _ = tables(rng, G, S, st.stride, goff)
    cap = n if cap is None else cap
    src = source(rng, st, pg, cap, n if count is None else count, form, E_in)
    mdt = np.uint8 if S <= 8 else np.uint16
    cut = np.where(rng.random((G, S)) < 0.2, 1 << np.arange(S), 0).sum(axis=1).astype(mdt)
    drop = np.where(rng.random(cap) < 0.15, rng.integers(1, 256, cap), 0).astype(np.uint8)
    c = SimpleNamespace(name=name, st=st, peer_group=pg, peer_from=pf, src=src, drop=drop, cut=cut,
                        ignore=(1 << 6) | (1 << 11), snap_status=snap_status, E_out=E_out,
                        stats=stats, form=form)
    c.want = carry(st, pg, pf, src, drop, cut, c.ignore, snap_status, E_out)
    return c


def cases():
    """Every length, batch size, slot count, run pair, offset and form of the issue, each
    value at least once with every length in both forms.  A case of 63 records or more must
    show all four dispositions and (with the flag) both status kinds: a case cannot silently
    cover nothing.  (A list of 0 or 1 records cannot hold six outcomes; those two lengths are
    exempt.)"""
    Es = ((0, 0), (1, 1), (0, 4), (4, 4))
    out = []
    for i, n in enumerate(LENGTHS):
        for j, form in enumerate(("outbox", "replies")):
            k = 2 * i + j
            out.append(make_case(f"n{n}-{form}", 7000 + k, n, (9, 69)[(i + j) % 2], (3, 9)[i % 2],
                                 Es[(i + j) % 4], (0, 1 << 40)[(k // 2 + j) % 2], form, k % 3 != 0))
    # the source's *count against its capacity: valid-looking records behind n; a count
    # above the capacity clips to it
    out.append(make_case("count-below-capacity", 7101, 200, 69, 9, (4, 4), 1 << 40, "outbox", True,
                         cap=333))
    out.append(make_case("count-above-capacity", 7102, 130, 9, 3, (1, 1), 0, "outbox", False,
                         cap=130, count=5000))
    out.append(make_case("flag-off", 7103, 129, 69, 3, (0, 4), 0, "replies", True,
                         snap_status=False))
    for c in out:
        w = c.want
        if w.n >= 63:
            assert set(np.unique(w.disposition)) == {LOCAL, REMOTE, LOST, BAD}, c.name
            kinds = set(np.unique(w.local["type"])) & {SNAP_STATUS, SNAP_STATUS_REJECT}
            assert kinds == ({SNAP_STATUS, SNAP_STATUS_REJECT} if c.snap_status else set()), c.name
    return out
