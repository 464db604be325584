"""tests/cluster_sim.py with duty H8, the vote half of H4 and MsgTimeoutNow
checked against qe_replies' rules: a backend that lists, after every
receiver-side call, the records the call's result rows ask for
(tests/replies_model.py on the models' outputs), and a Sim whose `send` holds
every response and vote message the host rules build against the record for
(sender group, slot, type).  Imports no torch."""
from collections import Counter

from tests import cluster_sim as cs
from tests import follower_model as fm
from tests import replies_model as rm
from tests import vote_model as vm


class RepliesMismatch(AssertionError):
    pass


def by_key(recs, goff):
    out = {(r["group"] - goff, r["to"], r["type"]): r for r in recs}
    assert len(out) == len(recs), "two records for one (group, slot, type)"
    return out


class ResultLog:
    """Mixin for a backend: `last` = (family, the result code of every group)
    of the newest receiver-side call, so that a Sim can name the kind of a
    message it sends."""

    last = (None, None)

    def follow(self, msgs):
        outs = super().follow(msgs)
        self.last = ("F", [o["result"] for o in outs])
        return outs

    def snap(self, msgs):
        outs = super().snap(msgs)
        self.last = ("S", [o["result"] for o in outs])
        return outs

    def vote(self, msgs):
        outs = super().vote(msgs)
        self.last = ("V", [o["result"] for o in outs])
        return outs


class ModelReplies(ResultLog, cs.ModelBackend):
    """ModelBackend whose receiver-side calls leave the model's records in
    `self.replies`, {(group, slot, type): record}; every record of a call must
    have been taken before the next call lists its own.  drop_hint: the
    negative control of tests/replies_model.build."""

    def __init__(self, p, drop_hint=False, **kw):
        super().__init__(p, **kw)
        self.replies, self.listed, self.drop_hint = {}, 0, drop_hint

    def list_records(self, **inp):
        if self.replies:
            raise RepliesMismatch(f"records no message was built for: {self.replies}")
        p, nodes = self.p, self.w.nodes
        st = rm.state(num_groups=p.G, group_offset=p.goff, num_slots=p.N, stride=p.stride,
                      last_index=[n.last_index() for n in nodes])
        recs, _ = rm.build(st, rm.inputs(term=[n.term for n in nodes], **inp), self.drop_hint)
        self.listed += len(recs)
        self.replies = by_key(recs, p.goff)

    @staticmethod
    def col(outs, k):
        return [o.get(k, 0) for o in outs]

    def follow(self, msgs):
        outs = super().follow(msgs)
        self.list_records(f_result=self.col(outs, "result"), f_from=[m.frm for m in msgs],
                          f_resp_index=self.col(outs, "resp_index"),
                          f_reject_hint=self.col(outs, "reject_hint"),
                          f_resp_log_term=self.col(outs, "resp_log_term"))
        return outs

    def snap(self, msgs):
        outs = super().snap(msgs)
        self.list_records(s_result=self.col(outs, "result"), s_from=[m.frm for m in msgs],
                          s_resp_index=self.col(outs, "resp_index"))
        return outs

    def vote(self, msgs):
        outs = super().vote(msgs)
        self.list_records(v_result=self.col(outs, "result"), v_type=[m.type for m in msgs],
                          v_from=[m.frm for m in msgs], v_resp_term=self.col(outs, "resp_term"),
                          v_req_log_term=self.col(outs, "req_log_term"),
                          v_req_to=self.col(outs, "req_to"))
        return outs

    def progress_step(self, mtype, mindex, mhint, mlogterm):
        o = super().progress_step(mtype, mindex, mhint, mlogterm)
        self.list_records(timeout_now=o.timeout_now)
        return o


F_KIND = {fm.FR_APP_ACCEPT: "app_accept", fm.FR_APP_STALE: "app_stale",
          fm.FR_APP_REJECT: "app_reject", fm.FR_LOWER_TERM_RESP: "app_lower_term",
          fm.FR_HEARTBEAT_RESP: "heartbeat_resp"}
KINDS = tuple(F_KIND.values()) + ("snap_resp", "vote_grant", "vote_reject", "prevote_resp",
                                  "vote_req", "prevote_req")
# what each of the two rows of tests/test_gpu_replies_cluster.py shows on the CPU
# models (tests/test_replies_model.py holds the counts): row "c" has no PreVote
REQUIRED_BY_ROW = {
    "c": tuple(k for k in KINDS if k not in ("prevote_resp", "prevote_req")),
    "b_small": KINDS,
}


class RepliesSim(cs.Sim):
    """Sim whose every R-class / V-class message is compared with the backend's
    record for (sender, slot, type): type, to, term, index, hint, log_term,
    flags.  With rebuild=True the message that goes on the network is rebuilt
    from the record, so what a node steps on is what the records say.  The
    local MsgSnapStatus (H11) is not a `send` and goes past untouched.
    `sent_cov` counts the kinds of message that went by."""

    def __init__(self, p, backend, rebuild=False, **kw):
        super().__init__(p, backend, **kw)
        self.rebuild, self.sent_cov = rebuild, Counter()

    def send(self, cls, frm_g, to_g, term, m):
        if cls in (cs.R_CLS, cs.V_CLS):
            term, m = self.check_record(cls, frm_g, to_g % self.p.N, term, m)
        super().send(cls, frm_g, to_g, term, m)

    def kind(self, cls, g, want):
        fam, results = self.be.last
        if cls == cs.R_CLS:
            assert fam in ("F", "S"), fam
            return F_KIND[results[g]] if fam == "F" else "snap_resp"
        assert fam == "V", fam
        if want["type"] in (rm.VOTE, rm.PREVOTE):
            return "vote_req" if want["type"] == rm.VOTE else "prevote_req"
        if want["type"] == rm.PREVOTE_RESP:
            return "prevote_resp"
        return "vote_reject" if want["flags"] & vm.VMF_REJECT else "vote_grant"

    def check_record(self, cls, g, s, term, m):
        p = self.p
        if cls == cs.R_CLS:
            t, index, hint, log_term = m
            want = dict(type=t + 3, index=index, hint=hint, log_term=log_term, flags=0)
        else:
            assert m.term == term, (m.term, term)
            want = dict(type=m.type + 10, index=m.index, hint=0, log_term=m.log_term,
                        flags=m.flags)
        want.update(group=p.goff + g, to=s, term=term, ctx=0)
        rec = self.be.replies.pop((g, s, want["type"]), None)
        if rec is None:
            raise RepliesMismatch(f"no record for the message of group {g} to slot {s}: {want}; "
                                  f"left: {self.be.replies}")
        got = {k: rec[k] for k in want}
        if got != want:
            raise RepliesMismatch(f"group {g} slot {s}: record {got}, the host rule builds {want}")
        self.sent_cov[self.kind(cls, g, want)] += 1
        if not self.rebuild:
            return term, m
        if cls == cs.R_CLS:
            return rec["term"], (rec["type"] - 3, rec["index"], rec["hint"], rec["log_term"])
        return rec["term"], vm.Msg(rec["type"] - 10, g % p.N, rec["term"], rec["index"],
                                   rec["log_term"], rec["flags"])

    def run(self):
        super().run()
        if self.be.replies:
            raise RepliesMismatch(f"records no message was built for: {self.be.replies}")
        return self
