"""tests/cluster_sim.py on the models alone (no GPU): the rows of
tests/test_gpu_cluster.py at the same seeds, sizes, rounds and fault settings,
a wider sweep of further seeds, and three negative controls that must break an
invariant.  What is proven here, before anything runs on a GPU: the invariants
(Election Safety, Monotonicity, Log Matching, State Machine Safety / Leader
Completeness) hold after every round, every cluster converges after the heal,
the run meets the coverage list of cluster_sim.required(), and the host layer
discards nothing but the kinds its docstring lists."""
import copy

import pytest

from tests import cluster_sim as cs
from tests import follower_model as fm
from tests import vote_model as vm

# the sweep: the rows' shapes with fewer clusters, 8 further seeds each
SWEEP = {"a": dict(C=30), "b": dict(C=6), "c": dict(fault_rounds=150)}
SWEEP_SEEDS = range(101, 109)


@pytest.mark.parametrize("name", sorted(cs.ROWS))
def test_gpu_rows_on_the_models(name):
    """The schedule the GPU test runs: invariants after every round and
    convergence (Sim.run raises otherwise), the coverage list, the discards."""
    sim = cs.Sim(cs.ROWS[name], cs.ModelBackend(cs.ROWS[name])).run()
    assert cs.missing(name, sim.cov) == []
    assert set(sim.discards) <= set(cs.HOST_DISCARDS)
    if cs.ROWS[name].base:  # the indices crossed 2^32
        assert all(n.committed > 1 << 32 for n in sim.w.nodes)


@pytest.mark.parametrize("name", sorted(cs.ROWS))
def test_sweep(name):
    """24 further seeds in all: the invariants and convergence at every seed;
    the coverage list over the row's seeds together (one small run need not
    meet every outcome)."""
    cov = cs.Counter()
    for seed in SWEEP_SEEDS:
        p = cs.ROWS[name].but(seed=seed, **SWEEP[name])
        sim = cs.Sim(p, cs.ModelBackend(p)).run()
        assert set(sim.discards) <= set(cs.HOST_DISCARDS)
        cov.update(sim.cov)
    assert cs.missing(name, cov) == []


# ---------------------------------------------------------------------------
# Negative controls: one rule broken each; check_invariants must notice.
# ---------------------------------------------------------------------------
def vote_ignoring_the_vote_row(node, m, *a):
    """Grants MsgVote whatever `vote` holds (raft.go:935-939 without its first
    two clauses): two candidates of one term both collect a quorum."""
    if m.type != vm.VMSG_VOTE or node.vote == fm.NONE_SLOT:
        return vm.step(node, m, *a)
    blank = copy.copy(node)
    blank.vote, blank.lead = fm.NONE_SLOT, fm.NONE_SLOT
    after, out = vm.step(blank, m, *a)
    return (node if after is blank else after), out


def follow_without_truncating(node, m, *a):
    """handleAppendEntries that overwrites from the conflict on but keeps the
    old entries past the message's last one (truncateAndAppend without the
    truncation)."""
    after, out = fm.step(node, m, *a)
    ci = out.get("append_from", 0)
    if out["result"] == fm.FR_APP_ACCEPT and ci and after.last_index() < node.last_index():
        bad = copy.deepcopy(after)
        bad.ents += [e for e in node.ents if e[0] > after.last_index()]
        bad.runs = fm.runs_of(bad.ents)
        if len(bad.runs) <= a[-1]:
            return bad, out
    return after, out


def run_until_broken(seeds, **kw):
    """-> the first InvariantError's text over the seeds (None: none broke).  A
    mutant may also run into a refusal the reference would panic on; that seed
    proves nothing and the next one is tried."""
    for seed in seeds:
        p = cs.ROWS["a"].but(seed=seed, C=12)
        be = cs.ModelBackend(p, **{k: v for k, v in kw.items() if k != "stale_resp_ok"})
        try:
            cs.Sim(p, be, stale_resp_ok=kw.get("stale_resp_ok", False)).run()
        except cs.InvariantError as e:
            return str(e)
        except AssertionError:
            continue
    return None


def test_negative_control_vote_row_ignored():
    """Breaks Election Safety."""
    err = run_until_broken(range(1, 9), vote_step=vote_ignoring_the_vote_row)
    assert err is not None and err.startswith("Election Safety"), err


def test_negative_control_append_without_truncation():
    """Breaks Log Matching (terms decrease along the log that kept its stale
    suffix) or commit safety."""
    err = run_until_broken(range(1, 9), follower_step=follow_without_truncating)
    assert err is not None and err.startswith(("Log Matching", "State Machine Safety")), err


def test_negative_control_stale_response_reaches_the_leader():
    """A host layer without the first rule of H6: a MsgAppResp of an earlier
    term reaches a leader's qe_progress_step and moves Match over entries the
    peer has lost since.  Over 60 seeds (and with delays up to 8 rounds and 30 %
    duplicates) this never broke commit safety: it needs the same node to lead
    twice with one peer truncated in between AND a quorum counted on that Match.
    What it does break is Convergence -- the leader believes the peer holds
    entries it lost and never sends them again -- at the seed pinned here.  The
    control that breaks Leader Completeness within the sweep is the next one."""
    err = run_until_broken([12], stale_resp_ok=True)
    assert err is not None and err.startswith("Convergence: committed"), err


def vote_without_the_log_check(node, m, *a):
    """Grants whatever the candidate's log (raft.go:940-942, isUpToDate,
    skipped): a node that misses committed entries is elected."""
    if m.type in (vm.VMSG_VOTE, vm.VMSG_PREVOTE):
        m = copy.copy(m)
        m.log_term = 1 << 62
    return vm.step(node, m, *a)


def test_negative_control_vote_without_up_to_date_check():
    """Replaces the stale-response control as the one that breaks Leader
    Completeness / State Machine Safety (the single rule broken: isUpToDate in
    the vote decision)."""
    err = run_until_broken(range(1, 9), vote_step=vote_without_the_log_check)
    assert err is not None and err.startswith(("Leader Completeness", "State Machine Safety",
                                               "Log Matching")), err
