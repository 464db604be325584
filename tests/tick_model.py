"""CPU restatement of raft.tick() for qe_tick (plain numpy, one function per
reference function, vectorised over the groups of a batch).  Independent of
the kernel: the counters are the reference's unbounded ints (packed with the
16-bit saturation only where the device form is compared), the hash is redone
in uint64 arithmetic, CheckQuorum and the beat walk the slots.

Reference: raft/raft.go tick functions :645-684, reset :597-599, promotable
:1618-1621, pastElectionTimeout / resetRandomizedElectionTimeout :1711-1720,
stepLeader's MsgBeat :991-993 and MsgCheckQuorum :997-1018, bcastHeartbeat
:524-541, sendHeartbeat :494-510, abortLeaderTransfer :1722-1724;
raft/tracker/tracker.go QuorumActive :215-225; raft/quorum majority.go
VoteResult :178-210, joint.go :61-75; raft/read_only.go
lastPendingRequestCtx :114-121."""
import numpy as np

FOLLOWER, CANDIDATE, LEADER, PRE_CANDIDATE = 0, 1, 2, 3
TEV_HEARD, TEV_RESET = 1, 2
HUP, BEAT, CHECKED_QUORUM, STEPDOWN, TRANSFER_ABORTED = 1, 2, 4, 8, 16
RECENT_ACTIVE = 8  # QE_PF_RECENT_ACTIVE of the packed peer word
NONE = 0xFF        # lead_transferee: no transfer in progress
PHI = np.uint64(0x9E3779B97F4A7C15)
DRAW_STREAM = 0x7131
ST_GROUPS, ST_ELECTIONS, ST_STEPDOWNS, ST_CHECKSUM = 0, 11, 13, 15
VOTE_PENDING, VOTE_LOST, VOTE_WON = 1, 2, 3


def mix64(z):
    """splitmix64 finalizer over a uint64 array (wrapping arithmetic)."""
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def hash4(seed, gid, lane, stream):
    k = np.uint64(((int(stream) & 0xFFFFFFFF) << 32) | (int(lane) & 0xFFFFFFFF))
    with np.errstate(over="ignore"):
        a = mix64(np.uint64(int(seed) & (2**64 - 1)) + np.asarray(gid, np.uint64) * PHI)
        return mix64(a ^ (k * np.uint64(0xD6E8FEB86659FD93)))


def draw(seed, gid, tick_no, et):
    """resetRandomizedElectionTimeout (:1718-1720): electionTimeout +
    Intn(electionTimeout), the Intn counter-based (h * et / 2^32 of the
    hash's upper word, done in Python ints)."""
    h = hash4(seed, gid, int(tick_no) & 0xFFFFFFFF, DRAW_STREAM) >> np.uint64(32)
    return np.array([et + ((int(x) * et) >> 32) for x in np.atleast_1d(h)], np.int64)


def majority_vote(member, voted, granted):
    """MajorityConfig.VoteResult over slot bitmaps (majority.go:178-210)."""
    def pc(x):  # popcount of slot bitmaps (non-negative, below 2^32)
        x = np.asarray(x, np.int64)
        assert ((x >= 0) & (x < 1 << 32)).all()
        return sum((x >> s) & 1 for s in range(32))
    n = pc(member)
    yes = pc(member & voted & granted)
    no = pc(member & voted & ~granted)
    missing = n - yes - no
    q = n // 2 + 1
    r = np.where(yes >= q, VOTE_WON, np.where(yes + missing >= q, VOTE_PENDING, VOTE_LOST))
    return np.where(n == 0, VOTE_WON, r)


def joint_vote(inc, out, voted, granted):
    """JointConfig.VoteResult (joint.go:61-75)."""
    r1, r2 = majority_vote(inc, voted, granted), majority_vote(out, voted, granted)
    return np.where(r1 == r2, r1,
                    np.where((r1 == VOTE_LOST) | (r2 == VOTE_LOST), VOTE_LOST, VOTE_PENDING))


class Model:
    """The tick state and the part of the leader state a tick touches, for G
    groups with S slots.  peer: uint32 [S][stride] packed words; match: uint64
    [S][stride]; masks int64 bitmaps or None as in qe_progress."""

    def __init__(self, G, S, et, ht, check_quorum, seed=0, goff=0, stride=None):
        self.G, self.S, self.et, self.ht = G, S, int(et), int(ht)
        self.check_quorum, self.seed, self.goff = bool(check_quorum), int(seed), int(goff)
        self.stride = stride or G
        self.tick_no = 0
        self.state = np.zeros(G, np.uint8)
        self.ee = np.zeros(G, np.int64)  # electionElapsed (an int, as in the reference)
        self.he = np.zeros(G, np.int64)  # heartbeatElapsed
        self.rt = np.full(G, self.et, np.int64)  # randomizedElectionTimeout
        self.no_campaign = np.zeros(G, np.uint8)
        self.peer = np.zeros(S * self.stride, np.uint32)
        self.match = np.zeros(S * self.stride, np.uint64)
        self.committed = np.zeros(G, np.uint64)
        self.inc = self.out = self.tracked = self.self_slot = None
        self.lead_transferee = None
        self.read_head = self.read_count = None
        self.read_cap = 4

    # -- the device form ----------------------------------------------------
    def timer(self):
        return (np.minimum(self.ee, 0xFFFF) | (np.minimum(self.he, 0xFFFF) << 16)).astype(np.uint32)

    def gid(self):
        return np.uint64(self.goff) + np.arange(self.G, dtype=np.uint64)

    def full(self):
        return np.full(self.G, (1 << self.S) - 1, np.int64)

    def masks(self):
        f = self.full()
        inc = f if self.inc is None else self.inc.astype(np.int64) & f
        out = np.zeros(self.G, np.int64) if self.out is None else self.out.astype(np.int64) & f
        trk = f if self.tracked is None else self.tracked.astype(np.int64) & f
        return inc, out, trk

    def self_bit(self):
        if self.self_slot is None:
            return np.zeros(self.G, np.int64)
        s = self.self_slot.astype(np.int64)
        return np.where(s < self.S, 1 << np.minimum(s, 62), 0)

    # -- reference functions ------------------------------------------------
    def reset_randomized_election_timeout(self, who):
        if who.any():
            self.rt[who] = draw(self.seed, self.gid()[who], self.tick_no, self.et)

    def reset(self, who):
        """The timer part of raft.reset() (:597-599)."""
        self.ee[who] = 0
        self.he[who] = 0
        self.reset_randomized_election_timeout(who)

    def apply_events(self, events):
        if events is None:
            return
        ev = np.asarray(events)
        self.ee[(ev & TEV_HEARD) != 0] = 0
        self.reset((ev & TEV_RESET) != 0)

    def promotable(self):
        """:1618-1621: a Progress of its own, not a learner, no pending snapshot."""
        inc, out, trk = self.masks()
        sb = self.self_bit()
        return ((sb & trk) != 0) & ((sb & (inc | out)) != 0) & (self.no_campaign == 0)

    def past_election_timeout(self):
        return self.ee >= self.rt

    def tick_election(self, who, action):
        self.ee[who] += 1
        hup = who & self.promotable() & self.past_election_timeout()
        # (for the tests' coverage: campaigns only a pending snapshot held back)
        nc, self.no_campaign = self.no_campaign, np.zeros_like(self.no_campaign)
        self.refused_by_snapshot = who & self.promotable() & self.past_election_timeout() & ~hup
        self.no_campaign = nc
        self.ee[hup] = 0
        action[hup] |= HUP  # the campaign itself is the caller's

    def step_check_quorum(self, who, action, quorum_active):
        """stepLeader MsgCheckQuorum (:997-1018) on the groups of `who` ->
        the groups whose quorum is not active."""
        inc, out, trk = self.masks()
        selft = self.self_bit() & trk
        pw = self.peer.reshape(self.S, self.stride)[:, : self.G]
        votes = np.zeros(self.G, np.int64)
        yes = np.zeros(self.G, np.int64)
        for s in range(self.S):
            tr = who & (((trk >> s) & 1) != 0)
            me = tr & (((selft >> s) & 1) != 0)
            pw[s, me] |= np.uint32(RECENT_ACTIVE)
            votes |= np.where(tr, 1 << s, 0)
            yes |= np.where(tr & ((pw[s] & RECENT_ACTIVE) != 0), 1 << s, 0)
        active = joint_vote(inc, out, votes, yes) == VOTE_WON
        for s in range(self.S):
            other = who & (((trk >> s) & 1) != 0) & (((selft >> s) & 1) == 0)
            pw[s, other] &= ~np.uint32(RECENT_ACTIVE)
        action[who] |= CHECKED_QUORUM
        quorum_active[who] = active[who]
        return who & ~active

    def abort_leader_transfer(self, who, action):
        if self.lead_transferee is None:
            return
        had = who & (self.lead_transferee < self.S)
        self.lead_transferee[had] = NONE
        action[had] |= TRANSFER_ABORTED

    def become_follower(self, who, action):
        """becomeFollower(r.Term, None) as far as the tick state goes: reset()
        clears the timers and the transfer."""
        self.state[who] = FOLLOWER
        self.reset(who)
        self.abort_leader_transfer(who, action)
        action[who] |= STEPDOWN

    def bcast_heartbeat(self, who, out):
        """bcastHeartbeat (:524-541): every Progress but the leader's gets
        Commit = min(Match, committed) and the newest pending context."""
        _, _, trk = self.masks()
        to = np.where(who, trk & ~self.self_bit(), 0)
        m = self.match.reshape(self.S, self.stride)[:, : self.G]
        if out.hb_commit is not None:
            hc = out.hb_commit.reshape(self.S, self.stride)[:, : self.G]
            for s in range(self.S):
                on = ((to >> s) & 1) != 0
                hc[s, on] = np.minimum(m[s, on], self.committed[on])
        ctx = np.zeros(self.G, np.uint32)
        if self.read_count is not None:
            q = np.minimum(self.read_count.astype(np.int64), self.read_cap)
            ctx = np.where(q > 0, (self.read_head.astype(np.int64) + q - 1) & 0xFFFFFFFF,
                           0).astype(np.uint32)
        out.hb_ctx[who] = ctx[who]
        out.hb_sent[:] = to

    def tick_heartbeat(self, who, action, out):
        self.he[who] += 1
        self.ee[who] += 1
        fire = who & (self.ee >= self.et)
        self.ee[fire] = 0
        if self.check_quorum:
            down = self.step_check_quorum(fire, action, out.quorum_active)
            self.become_follower(down, action)
        still = fire & (self.state == LEADER)
        self.abort_leader_transfer(still, action)
        lead = who & (self.state == LEADER)
        beat = lead & (self.he >= self.ht)
        self.he[beat] = 0
        action[beat] |= BEAT
        self.bcast_heartbeat(beat, out)

    def tick(self, events=None, out=None, ticks=1):
        """One qe_tick call -> TickOut (out: prefilled arrays kept where the
        tick writes nothing)."""
        out = out or TickOut(self)
        action = np.zeros(self.G, np.uint8)
        self.apply_events(events)
        out.hb_sent[:] = 0
        if ticks:
            leader = self.state == LEADER
            self.tick_election(~leader, action)
            self.tick_heartbeat(leader, action, out)
        out.action[:] = action
        out.stats = self.stats(action)
        self.tick_no += ticks
        return out

    def stats(self, action):
        st = np.zeros(16, np.uint64)
        st[ST_GROUPS] = self.G
        st[ST_ELECTIONS] = int(((action & HUP) != 0).sum())
        st[ST_STEPDOWNS] = int(((action & STEPDOWN) != 0).sum())
        with np.errstate(over="ignore"):
            x = (self.gid() * PHI) ^ np.uint64(0xA0761D6478BD642F) ^ \
                (action.astype(np.uint64) << np.uint64(56)) ^ \
                (self.rt.astype(np.uint64) << np.uint64(32)) ^ self.timer().astype(np.uint64)
            st[ST_CHECKSUM] = np.add.reduce(mix64(x))
        return st


class TickOut:
    def __init__(self, m, sentinel=0):
        md = np.uint8 if m.S <= 8 else np.uint16
        self.action = np.zeros(m.G, np.uint8)
        self.hb_commit = np.full(m.S * m.stride, sentinel, np.uint64)
        self.hb_ctx = np.full(m.G, sentinel & 0xFFFFFFFF, np.uint32)
        self.hb_sent = np.zeros(m.G, md)
        self.quorum_active = np.full(m.G, sentinel & 0xFF, np.uint8)
        self.stats = None
