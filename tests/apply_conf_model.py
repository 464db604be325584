"""Sequential model of qe_apply_conf (include/etcd_quorum.h, rules 1-6): a
list of committed conf-change entries applied as RawNode.ApplyConfChange does,
record by record in list order.

* the Changer is oracle/confchange_ref.py, keyed by ID.  SlotChanger adds the
  one thing the slot model decides and the reference does not: which slot a
  created Progress takes (the lowest untracked one, or the slot the change
  names);
* decode() is ConfChangeV2.LeaveJoint / EnterJoint (raft/raftpb/confchange.go:
  71-107);
* a leader's half of switchToConfig is orc.switch_config, run once after the
  list on the groups a leader applied a record for (a group takes part with
  one record at most, so the order among groups is free).

TEST INFRASTRUCTURE ONLY.  tests/test_apply_conf_model.py pins it to the
reference's interaction traces.
"""
import numpy as np

from oracle import confchange_ref as cc

AUTO, JOINT_IMPLICIT, JOINT_EXPLICIT = 0, 1, 2
ANY_SLOT = 0xFF
APPLIED, LEADER, DEFERRED = 1, 2, 3
REFUSED = 16
BAD_GROUP, BAD_ORDER, BAD_CHANGE, CHANGER_ERROR, SKIPPED = 16, 17, 18, 19, 20
PR_PROBE, PF_RECENT_ACTIVE = 0, 8


def decode(transition, count):
    """Rule 1 -> the Changer operation."""
    if count == 0 and transition == AUTO:
        return cc.OP_LEAVE_JOINT
    if transition != AUTO or count > 1:
        return cc.OP_ENTER_JOINT_AUTO if transition != JOINT_EXPLICIT else cc.OP_ENTER_JOINT
    return cc.OP_SIMPLE


class SlotChanger(cc.Changer):
    """cc.Changer whose changes are (type, node, slot) and whose Progress map
    is placed in S slots: `slots` maps every id that holds a Progress to its
    slot."""

    def __init__(self, S, cfg=None, prs=None, slots=None, last_index=0):
        super().__init__(cfg, prs, last_index)
        self.S, self.slots = S, dict(slots or {})
        self._work, self._want = None, ANY_SLOT

    def _apply(self, cfg, prs, ccs):  # :152-177, one change at a time for its slot
        for typ, node, want in ccs:
            self._want = want
            if node == 0:
                continue
            if typ == cc.ADD_NODE:
                self._make_voter(cfg, prs, node)
            elif typ == cc.ADD_LEARNER_NODE:
                self._make_learner(cfg, prs, node)
            elif typ == cc.REMOVE_NODE:
                self._remove(cfg, prs, node)
            elif typ != cc.UPDATE_NODE:
                raise cc.ChangeError(cc.ERR_BAD_TYPE)
        if not cfg.inc:
            raise cc.ChangeError(cc.ERR_REMOVED_ALL)

    def _init_progress(self, cfg, prs, i, is_learner):
        used = {self._work[j] for j in prs}
        if self._want == ANY_SLOT:
            free = [s for s in range(self.S) if s not in used]
            if not free:
                raise cc.ChangeError(cc.ERR_NO_SLOT)
            s = free[0]
        else:
            if self._want >= self.S or self._want in used:
                raise cc.ChangeError(cc.ERR_NO_SLOT)
            s = self._want
        self._work[i] = s
        self.created.add(i)
        super()._init_progress(cfg, prs, i, is_learner)

    def run(self, op, ccs):
        """-> QE_CC_*; on success self.created holds the ids whose Progress the
        operation created and still holds."""
        self._work, self.created = dict(self.slots), set()
        rc = super().run(op, ccs)
        if rc == cc.OK:
            self.slots = {i: self._work[i] for i in self.prs}
            self.created &= set(self.prs)
        else:
            self.created = set()
        return rc

    def mask(self, ids):
        m = 0
        for i in ids:
            m |= 1 << self.slots[i]
        return m

    def conf_state(self, created=()):
        """The record's ConfState in slot form (rule 6)."""
        c = self.cfg
        ids = [0] * self.S
        for i, s in self.slots.items():
            ids[s] = i
        return {"inc": self.mask(c.inc), "out": self.mask(c.out), "learner": self.mask(c.learners),
                "learners_next": self.mask(c.lnext), "tracked": self.mask(self.prs),
                "new_progress": self.mask(created), "auto_leave": int(c.auto_leave), "ids": ids}


EMPTY = {"inc": 0, "out": 0, "learner": 0, "learners_next": 0, "tracked": 0, "new_progress": 0,
         "auto_leave": 0}


class Model:
    """G groups: changers[g] (SlotChanger), leader[g]; `pb` (orc.ProgressBatch,
    optional) holds the Progress rows, the masks a leader's switch reads and
    last_index.  Without pb the Changer's LastIndex is last_index[g] of the
    constructor (default 0) and no switch runs."""

    def __init__(self, G, S, goff=0, max_changes=255, pb=None, decode=decode):
        self.G, self.S, self.goff, self.C, self.pb = G, S, goff, max_changes, pb
        self.decode = decode
        self.changers = [SlotChanger(S) for _ in range(G)]
        self.leader = [False] * G

    def _sync(self, g, created):
        """The group's configuration into pb's masks, initProgress for the
        created slots (raft/confchange/confchange.go:251-274)."""
        pb, ch = self.pb, self.changers[g]
        pb.inc[g], pb.out[g] = ch.mask(ch.cfg.inc), ch.mask(ch.cfg.out)
        pb.tracked[g] = ch.mask(ch.prs)
        for i in created:
            k = ch.slots[i] * pb.stride + g
            pb.match[k], pb.next[k], pb.pending[k] = 0, pb.last_index[g], 0
            pb.pw[k] = PR_PROBE | PF_RECENT_ACTIVE

    def apply(self, records, capacity=None):
        """records: (group, transition, count, [(type, node, slot), ...]) in
        list order -> one dict per record of the first min(n, capacity):
        result, cc_result, sw_result (0 until switch()), and the ConfState."""
        n = len(records) if capacity is None else min(len(records), capacity)
        out = []
        switched = np.zeros(self.G, np.uint8)
        i = 0
        while i < n:
            gid = records[i][0]
            j = i
            while j < n and records[j][0] == gid:
                j += 1
            g = gid - self.goff
            head = (BAD_ORDER if i > 0 and gid < records[i - 1][0] else
                    BAD_GROUP if not 0 <= g < self.G else 0)
            if head:
                for k in range(i, j):
                    out.append(dict(EMPTY, ids=[0] * self.S, result=head if k == i else SKIPPED,
                                    cc_result=0, sw_result=0, group=gid))
                i = j
                continue
            ch = self.changers[g]
            refused = led = False
            for k in range(i, j):
                _, tr, cnt, ccs = records[k]
                res, ccr, created = 0, 0, ()
                if refused:
                    res = SKIPPED
                elif led:
                    res = DEFERRED
                elif tr > JOINT_EXPLICIT or cnt > self.C:
                    res = BAD_CHANGE
                else:
                    if self.pb is not None:
                        ch.last_index = int(self.pb.last_index[g])
                    ccr = ch.run(self.decode(tr, cnt), list(ccs)[:cnt])
                    if ccr != cc.OK:
                        res = CHANGER_ERROR
                    else:
                        created = set(ch.created)
                        res = LEADER if self.leader[g] else APPLIED
                        led = self.leader[g]
                        if self.pb is not None:
                            self._sync(g, created)
                refused = refused or res >= REFUSED
                out.append(dict(ch.conf_state(created), result=res, cc_result=ccr, sw_result=0,
                                group=gid))
            if led:
                switched[g] = 1
            i = j
        self.switched = switched
        return out

    def switch(self, out):
        """The leader half after the list: orc.switch_config on the groups a
        leader applied a record for; fills sw_result.  -> orc.SwitchOut."""
        from oracle import orc
        o = orc.switch_config(self.pb, self.switched, self.goff)
        for r in out:
            if r["result"] == LEADER:
                r["sw_result"] = int(o.result[r["group"] - self.goff])
        return o
