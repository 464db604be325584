"""A row-level Python restatement of qe_read_note and qe_read_states
(include/etcd_quorum.h, rules 1-9): what the kernels compute, from the same
rows, one group at a time.  It is the checker of the GPU tests
(tests/test_gpu_read_states.py) and is itself held against an independent
read_only.go kept as Python lists (tests/test_read_states_model.py)."""
import numpy as np

M32, M64 = (1 << 32) - 1, (1 << 64) - 1
PHI, SALT = 0x9E3779B97F4A7C15, 0xE7037ED1A0B428DB
RI_RESPOND, RI_QUEUED = 1, 3
RS_STATE, RS_RESP, RS_TERM_COMMIT = 1, 2, 3
READ_QUEUE = 4
STAT_GROUPS, STAT_STATE, STAT_RESP, STAT_TERM_COMMIT, STAT_CHECKSUM = 0, 4, 6, 9, 15
BY_KIND = {RS_STATE: STAT_STATE, RS_RESP: STAT_RESP, RS_TERM_COMMIT: STAT_TERM_COMMIT}
FIELDS = ("group", "kind", "to", "ctx", "index", "key")


def mix64(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def book_cap(read_cap):
    return read_cap if read_cap else READ_QUEUE


class Book:
    """qe_read_book as numpy rows [G][cap]."""

    def __init__(self, G, read_cap):
        self.G, self.cap = G, book_cap(read_cap)
        self.req_index = np.zeros(G * self.cap, np.uint64)
        self.req_from = np.full(G * self.cap, 0xFF, np.uint8)


def read_note(book, result, ctx, index, from_=None):
    """qe_read_note: a QUEUED request's index and origin at ctx % cap."""
    cap = book.cap
    for g in np.nonzero(np.asarray(result) == RI_QUEUED)[0]:
        e = int(g) * cap + int(ctx[g]) % cap
        book.req_index[e] = index[g]
        book.req_from[e] = 0xFF if from_ is None else from_[g]


def kind_of(f, self_slot, S):
    """Rule 3 -> (kind, to)."""
    if f >= S or f == self_slot:
        return RS_STATE, 0xFF
    return RS_RESP, f


def read_states(G, S, read_cap, read_head, book=None, self_slot=None, read_keys=None,
                group_offset=0, read_released=None, term_commit=None, term_commit_index=None,
                ri_result=None, ri_index=None, ri_from=None, ri_key=None):
    """qe_read_states -> (the full list of records as dicts, stats[16])."""
    cap = book_cap(read_cap)
    recs, stats = [], [0] * 16
    for g in range(G):
        gid = group_offset + g
        me = 0xFF if self_slot is None else int(self_slot[g])
        mine = []
        k = 0 if read_released is None else int(read_released[g])
        for j in range(k):  # rule 2: oldest first
            c = (int(read_head[g]) - k + j) & M32
            e = g * cap + c % cap
            kind, to = kind_of(int(book.req_from[e]), me, S)
            mine.append(dict(group=gid, kind=kind, to=to, ctx=c, index=int(book.req_index[e]),
                             key=0 if read_keys is None else int(read_keys[e])))
        if term_commit is not None and term_commit[g]:  # rule 4
            mine.append(dict(group=gid, kind=RS_TERM_COMMIT, to=0xFF, ctx=0,
                             index=int(term_commit_index[g]), key=0))
        if ri_result is not None and ri_result[g] == RI_RESPOND:  # rule 5
            kind, to = kind_of(0xFF if ri_from is None else int(ri_from[g]), me, S)
            mine.append(dict(group=gid, kind=kind, to=to, ctx=0, index=int(ri_index[g]),
                             key=0 if ri_key is None else int(ri_key[g])))
        stats[STAT_GROUPS] += 1 if mine else 0
        for r in mine:
            stats[BY_KIND[r["kind"]]] += 1
            h = mix64((r["group"] * PHI) ^ SALT ^ (r["kind"] << 56) ^ (r["to"] << 48) ^ r["ctx"])
            h = mix64(mix64(h ^ r["index"]) ^ r["key"])
            stats[STAT_CHECKSUM] = (stats[STAT_CHECKSUM] + h) & M64
        recs += mine
    return recs, stats


def columns(recs, n=None):
    """The first n records as the arrays the call fills."""
    recs = recs if n is None else recs[:n]
    dt = dict(group=np.uint64, kind=np.uint8, to=np.uint8, ctx=np.uint32, index=np.uint64,
              key=np.uint64)
    return {k: np.array([r[k] for r in recs], dt[k]) for k in FIELDS}
