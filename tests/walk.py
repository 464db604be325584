"""The walking-wave shape of the one-lane-per-group kernels' GPU tests.

With statistics the grid of qe_tick, qe_follower_step, qe_vote_step,
qe_snapshot_step and qe_compact is capped at 8 blocks (32 waves, one 64-group
tile each) per CU and the waves walk.  walk_groups() is a batch in which every
wave walks two tiles, two waves walk three and the last tile is ragged, so the
tile loop, the per-wave counters carried across tiles and the partial tile of
a walk all run.  The Python models step a node at a time, so the state is a
base of PERIOD groups repeated: every row of the result is the base's
expectation repeated and every counter but the checksum the repeated base's
sum.  The checksum depends on the group id; the models restate their per-group
hash over arrays (group_hashes / step_hashes / compact_hashes), and
tests/test_walk_model.py pins those to the scalar functions on the base.

The bases are built once per process and never modified."""
import functools

import numpy as np

from tests import follower_model as fm
from tests import snapshot_model as sm
from tests import vote_model as vm

PERIOD = 209             # groups of a base: 3 tiles and 17 lanes, coprime to 64
GOFF = (1 << 33) + 4099  # group_offset: the checksum's group ids pass 2^32
PAD = 11                 # stride - G (G % 64 == 21: the stride is no multiple of 64)
R, S, E = 4, 5, 1        # the smallest log and mask shapes: one bucket, u8 masks
SENT = 0x0E0E0E0E0E0E0E0E
CSUM = 15                # QE_STAT_CHECKSUM


def walk_groups(cus):
    """(2 * cap + 2) tiles and 21 groups, cap = the capped grid's wave count."""
    cap = cus * 8 * 4
    return (2 * cap + 2) * 64 + 21


OPEN, HOT, LONE, OUT = range(4)
CHUNK = 4096             # records per chunk of a record list's count, scan and fill


def three_chunks():
    """The shape of the deferred-positions lists of tests/test_gpu_inbox.py and
    tests/test_gpu_requests.py: 3 * CHUNK + 1 records over G = 4200 groups ->
    (G, role[n], group[n] before the group offset).  A test turns the roles into records of its
    call: OPEN the first record of a hot group (0..63), which it closes; HOT a
    later record of a hot group, so DEFERRED; LONE the one record of its group
    (64..4159), whatever it is; OUT a record outside the batch (group G + 1).
    Tile 0 opens the hot groups, tile 1 is all HOT, the rest of chunk 0 and
    chunk 2 are HOT or OUT at random with records 4095, 8192 and 12288 HOT, and
    chunk 1 is all LONE."""
    n, G = 3 * CHUNK + 1, 64 + CHUNK + 40
    rng = np.random.default_rng(4095)
    role = np.where(rng.random(n) < 0.5, HOT, OUT)
    role[:64], role[64:128], role[CHUNK:2 * CHUNK] = OPEN, HOT, LONE
    role[[CHUNK - 1, 2 * CHUNK, 3 * CHUNK]] = HOT
    i = np.arange(n)
    group = np.select([role == LONE, role == OUT], [64 + i - CHUNK, G + 1], i % 64)
    return G, role, group


def check_three_chunks(deferred, group):
    """What the lists of three_chunks() are for, asserted on a model's deferred
    list: (a) record 4095, the last lane of the last tile of chunk 0, is
    deferred; (b) no record of chunk 1 is, and each goes to a group no other
    record touches; (c) record 8192, the first of chunk 2, is; (d) record 12288,
    the lone record of the ragged last chunk, is; (e) a tile of chunk 0 holds no
    deferred record and one holds 64."""
    n = 3 * CHUNK + 1
    flag = np.zeros(n, bool)
    flag[np.asarray(deferred, np.int64)] = True
    assert len(group) == n and flag[CHUNK - 1] and flag[2 * CHUNK] and flag[3 * CHUNK]
    assert not flag[CHUNK:2 * CHUNK].any()
    assert (np.bincount(group)[group[CHUNK:2 * CHUNK]] == 1).all()
    per_tile = flag[:CHUNK].reshape(-1, 64).sum(axis=1)
    assert (per_tile == 0).any() and (per_tile == 64).any()
    assert flag[2 * CHUNK + 1:3 * CHUNK].any() and not flag[2 * CHUNK + 1:3 * CHUNK].all()


def repeat(arrays, G, stride, rows=(), fill=0):
    """The base's packed arrays (dict, base stride PERIOD) with period PERIOD
    up to G groups.  rows: {name: row count} of the [rows][stride] arrays, or
    {name: (row count, stride)} for one with a stride of its own; their pad
    columns hold `fill`."""
    idx = np.arange(G) % PERIOD
    rows = dict(rows)
    out = {}
    for k, a in arrays.items():
        if a is None:
            out[k] = None
        elif k in rows:
            n, st = rows[k] if isinstance(rows[k], tuple) else (rows[k], stride)
            big = np.full((n, st), fill, a.dtype)
            big[:, :G] = a.reshape(n, PERIOD)[:, idx]
            out[k] = big.reshape(-1)
        else:
            out[k] = a[idx]
    return out


def gids(G):
    return np.uint64(GOFF) + np.arange(G, dtype=np.uint64)


def expect_stats(shares, G, hashes):
    """The folded statistics of the repeated base: shares[j] is the model's
    stats dict of base group j (None without a message), hashes the per-group
    checksum terms of all G groups."""
    idx = np.arange(G) % PERIOD
    cnt = np.bincount(idx, minlength=PERIOD)
    ws = [0] * 16
    for j, s in enumerate(shares):
        for k, v in (s or {}).items():
            if k != CSUM:
                ws[k] += int(v) * int(cnt[j])
    has = np.array([s is not None for s in shares])[idx]
    with np.errstate(over="ignore"):
        ws[CSUM] = int(np.add.reduce(hashes[has]))
    return np.array([w & fm.M64 for w in ws], np.uint64)


class Base:
    pass


@functools.lru_cache(maxsize=None)
def follower_base(flags=3):
    b = Base()
    rng = np.random.default_rng(2091)
    b.flags = flags
    b.nodes = [fm.gen_node(rng, R, S) for _ in range(PERIOD)]
    b.msgs = [fm.gen_msg(rng, n, E, S) for n in b.nodes]
    b.after, b.outs, _ = fm.step_batch(b.nodes, b.msgs, flags, S, R)
    b.shares = [fm.group_stats(0, n, n2, o) if m.type != fm.LMSG_NONE else None
                for n, n2, o, m in zip(b.nodes, b.after, b.outs, b.msgs)]
    return b


@functools.lru_cache(maxsize=None)
def vote_base(flags=3, et=10):
    b = Base()
    rng = np.random.default_rng(2092)
    b.flags, b.et = flags, et
    b.nodes = [vm.gen_node(rng, R, S, "inc", et) for _ in range(PERIOD)]
    b.msgs = [vm.gen_msg(rng, n, S) for n in b.nodes]
    b.after, b.outs, _ = vm.step_batch(b.nodes, b.msgs, flags, S, et)
    b.shares = [vm.group_stats(0, n2, o) if m.type != vm.VMSG_NONE else None
                for n2, o, m in zip(b.after, b.outs, b.msgs)]
    return b


@functools.lru_cache(maxsize=None)
def snap_base():
    b = Base()
    rng = np.random.default_rng(2093)
    b.nodes = [sm.gen_snode(rng, R, S) for _ in range(PERIOD)]
    b.msgs = [sm.gen_smsg(rng, n, S) for n in b.nodes]
    b.after, b.outs, _ = sm.step_batch(b.nodes, b.msgs, S, R)
    b.shares = [sm.step_stats(0, n, n2, o) if m.type != sm.SMSG_NONE else None
                for n, n2, o, m in zip(b.nodes, b.after, b.outs, b.msgs)]
    return b


@functools.lru_cache(maxsize=None)
def compact_base():
    b = Base()
    rng = np.random.default_rng(2094)
    b.nodes = [sm.gen_snode(rng, R, S) for _ in range(PERIOD)]
    b.reqs = [sm.gen_compaction(rng, n) for n in b.nodes]
    b.after, b.outs, _ = sm.compact_batch(b.nodes, b.reqs)
    b.shares = [sm.compact_stats(0, n2, o) if (ci or si) else None
                for n2, o, (ci, si, _) in zip(b.after, b.outs, b.reqs)]
    return b


# The checksum terms of G groups from the packed state after the step and the
# results (arrays of G groups each; gid defaults to the walk's).
def follower_hashes(want, result, gid=None):
    gid = gids(len(result)) if gid is None else gid
    return fm.group_hashes(gid, result, want["term"], want["committed"], want["last_index"])


def vote_hashes(want, result, events, gid=None):
    gid = gids(len(result)) if gid is None else gid
    return vm.group_hashes(gid, result, want["term"], want["state"], want["lead"], want["vote"],
                           events, want["voted"], want["granted"])


def snap_hashes(want, result, gid=None):
    gid = gids(len(result)) if gid is None else gid
    return sm.step_hashes(gid, result, want["term"], want["committed"], want["last_index"])


def compact_hashes(want, result, gid=None):
    gid = gids(len(result)) if gid is None else gid
    dummy = want["run_first"].reshape(R, -1)[0, :len(result)]  # the dummy entry's row
    return sm.compact_hashes(gid, result, dummy, want["run_count"], want["snap_index"])
