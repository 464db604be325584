"""qe_tune("tiles_per_wave") and the persistent grid on the Progress side.

The chunked launchers, qe_progress_send, qe_check_quorum and qe_confchange,
give each wave a chunk of tiles (etcd_amd/csrc/qe_launch.hpp); an override is
floored at 2 and clamped to the kernel's 8.

Every other Progress kernel (k_progress_step in each of its forms, k_propose,
k_switch_config, k_become_leader, k_read_index) takes one 64-group tile per
wave by default and loops `for (t = wave; t < ntiles; t += nwaves)` when the
launch plan says so: tiles_per_wave = T > 0 gives every wave T tiles,
tiles_per_wave = 0 the persistent grid of blocks_per_cu blocks per CU.  The
code that runs only from the second iteration on (the prefetch of the next
tile's header, the per-wave LDS reused by the next tile, the counters and the
byte count carried over the walk) runs here: at 3001 groups, 47 tiles, under 2
(23 waves walk two tiles and the last finds none), 3 (a ragged third step) and
64 (one block whose four waves walk 11-12 tiles each), and on the persistent
grid of one block per CU at a batch in which every wave walks two or three
tiles and the last tile is ragged.

Whatever the plan, the outputs, the state, the folded statistics and the byte
count are the oracle's (the differentials of the kernels' own test files, run
again under each plan), and the same bits as the default plan's."""
import copy

import numpy as np
import pytest
import torch

from oracle import confchange_ref as cc
from oracle import orc
from tests.test_gpu_confchange import run_differential
from tests.test_gpu_progress import (DEV, EXTRAS, assert_same, random_state, rounds_vs_oracle,
                                     to_dev_mask, to_device)
from tests.test_gpu_propose import propose_vs_oracle
from tests.test_gpu_readindex import deep_queues_vs_oracle
from tests.test_gpu_switch import become_leader_vs_oracle, switch_vs_oracle

pytestmark = pytest.mark.gpu
G = 323  # five full tiles and a ragged one of 3 lanes
TPW = [-1, 1, 2, 3, 8, 9]  # default; floored to 2; 2; odd; the kernels' maximum; clamped to 8


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from etcd_amd import engine
    return engine


def same_arrays(a, b, what):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for k in a:
            same_arrays(a[k], b[k], f"{what}.{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            same_arrays(x, y, f"{what}[{i}]")
    elif a is None or np.isscalar(a):
        assert a == b, what
    else:
        np.testing.assert_array_equal(a, b, err_msg=what)


@pytest.mark.parametrize("S,masks", [(3, ()), (9, ("inc", "out"))])
def test_send_and_check_quorum_under_tiles_per_wave(eng, S, masks):
    rng = np.random.default_rng(7700 + S)
    md = orc.mask_dtype(S)
    pb0 = random_state(rng, G, S, 8, 2, masks, EXTRAS, max_ents=2)
    want = rng.integers(0, 1 << S, G).astype(md)
    # the oracle, once
    pb_send = copy.deepcopy(pb0)
    o_sent, o_snap = orc.progress_send(pb_send, want, 1)
    pb_cq = copy.deepcopy(pb_send)
    o_qa, o_st = orc.check_quorum(pb_cq)
    first = None
    try:
        for tpw in TPW:
            eng.tune("tiles_per_wave", tpw)
            ps = to_device(eng, copy.deepcopy(pb0), masks, EXTRAS)
            sent, snap = eng.progress_send(ps, to_dev_mask(want, S), 1)
            sent, snap = sent.cpu().numpy().view(md), snap.cpu().numpy().view(md)
            np.testing.assert_array_equal(sent, o_sent, err_msg=f"sent, tpw {tpw}")
            np.testing.assert_array_equal(snap, o_snap, err_msg=f"snap, tpw {tpw}")
            assert_same(ps, pb_send)
            after_send = ps.host()
            st = eng.stats_buffer(DEV)
            qa = eng.check_quorum(ps, stats=st).cpu().numpy()
            got = eng.stats_reduce(st).cpu().numpy().view(np.uint64)
            np.testing.assert_array_equal(qa, o_qa, err_msg=f"quorum_active, tpw {tpw}")
            np.testing.assert_array_equal(got, o_st, err_msg=f"stats, tpw {tpw}")
            assert_same(ps, pb_cq)
            run = (sent, snap, after_send, qa, got, ps.host())
            if first is None:
                first = run
            same_arrays(run, first, f"tpw {tpw} against tpw {TPW[0]}")
    finally:
        eng.tune("tiles_per_wave", -1)


@pytest.mark.parametrize("S", [3, 9])
def test_confchange_under_tiles_per_wave(eng, S):
    first = None
    try:
        for tpw in TPW:
            eng.tune("tiles_per_wave", tpw)
            trace = []
            seen = run_differential(eng, S, S, G, 4, 7800 + S, trace=trace)  # against the oracle
            assert cc.OK in seen
            if first is None:
                first = trace
            same_arrays(trace, first, f"tpw {tpw} against tpw {TPW[0]}")
    finally:
        eng.tune("tiles_per_wave", -1)


# ---- the one-tile-per-wave kernels: (name, tiles_per_wave, blocks_per_cu) ----
G_WALK = 3001  # 47 tiles
DEFAULT = ("default", -1, 0)
WALK = [DEFAULT, ("tiles_per_wave 2", 2, 0), ("tiles_per_wave 3", 3, 0), ("tiles_per_wave 64", 64, 0)]
PERSISTENT = [DEFAULT, ("persistent grid, 1 block per CU", 0, 1)]


def persistent_groups():
    """(2 * waves + 2) tiles and 21 groups, waves = the persistent grid's at one
    block per CU: every wave walks two tiles, the first walk three, and the last
    tile is ragged."""
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    return (2 * cus * 4 + 2) * 64 + 21


def under_plans(eng, plans, run):
    """run(trace) under each launch plan: it asserts the oracle's bits itself
    and appends what the device produced to `trace`; every plan's trace must
    equal the default plan's."""
    first = None
    try:
        for name, tpw, bpc in plans:
            eng.tune("tiles_per_wave", tpw)
            eng.tune("blocks_per_cu", bpc)
            trace = []
            try:
                run(trace)
            except AssertionError as err:
                raise AssertionError(f"plan '{name}' against the oracle: {str(err).strip()}") from err
            assert trace, name
            if first is None:
                first = trace
            same_arrays(trace, first, f"plan '{name}' against plan '{plans[0][0]}'")
    finally:
        eng.tune("tiles_per_wave", -1)
        eng.tune("blocks_per_cu", 0)


#              S  masks           extras  R  F   ring16
STEP_CASES = [(5, (),             (),     3, 8,  False),  # pipelined, rings in row form
              (5, ("inc",),       EXTRAS, 3, 8,  False),  # the same with reads (RD)
              (10, ("inc", "out"), (),    3, 8,  False),  # rolled: S = 10
              (5, (),             EXTRAS, 3, 32, False),  # rolled: memory rings
              (5, (),             EXTRAS, 6, 8,  False),  # the 8-run kernel
              (5, (),             EXTRAS, 9, 8,  False),  # the 16-run kernel, one wave per block
              (5, (),             (),     3, 8,  True),   # 16-bit rings, the four-wave kernel
              (5, ("inc",),       EXTRAS, 3, 8,  True),   # 16-bit rings with reads
              (7, ("inc", "out"), EXTRAS, 3, 5,  True)]   # 16-bit rings, joint
STEP_IDS = ["pipelined", "pipelined-reads", "rolled-S10", "rolled-F32", "runs8", "runs16",
            "ring16", "ring16-reads", "ring16-joint"]


@pytest.mark.parametrize("S,masks,extras,R,F,ring16", STEP_CASES, ids=STEP_IDS)
def test_progress_step_waves_walk(eng, S, masks, extras, R, F, ring16):
    """The rounds of tests/test_gpu_progress.py (odd rounds the instrumented
    variant, whose byte count is carried over the walk; qe_read_index between
    rounds where the state has a queue) with every wave of qe_progress_step
    walking 2, 3 and 11-12 tiles."""
    under_plans(eng, WALK, lambda trace: rounds_vs_oracle(eng, S, masks, extras, R, F, ring16,
                                                          G=G_WALK, trace=trace))


# (the rolled form with 3-entry rings: at this batch size the host copies of
#  8- and 32-entry rings of 10 slots alone cost seconds)
PERSISTENT_STEP = ([(c, i) for c, i in zip(STEP_CASES, STEP_IDS) if not i.startswith("rolled")] +
                   [((10, ("inc", "out"), (), 3, 3, False), "rolled-S10-F3")])


@pytest.mark.parametrize("S,masks,extras,R,F,ring16", [c for c, _ in PERSISTENT_STEP],
                         ids=[i for _, i in PERSISTENT_STEP])
def test_progress_step_persistent_grid(eng, S, masks, extras, R, F, ring16):
    """The first two of those rounds (a plain and an instrumented step, two
    sends and a CheckQuorum) on the persistent grid, in every form of the
    kernel."""
    G = persistent_groups()
    under_plans(eng, PERSISTENT, lambda trace: rounds_vs_oracle(eng, S, masks, extras, R, F, ring16,
                                                                G=G, rounds=2, trace=trace))


def test_read_index_deep_queues_waves_walk(eng):
    """qe_read_index and the step on queues past the word (cap 64), three
    tiles per wave."""
    under_plans(eng, [DEFAULT, WALK[2]],
                lambda trace: deep_queues_vs_oracle(eng, 5, ("inc",), 64, 8, trace=trace))


@pytest.mark.parametrize("S,F,masks,extras,max_cc,max_ents,ring16", [
    (5, 8, ("inc", "out"), EXTRAS, 3, 2, False), (9, 8, ("inc", "out"), EXTRAS, 3, 2, True)],
    ids=["ring32", "ring16"])
def test_propose_waves_walk(eng, S, F, masks, extras, max_cc, max_ents, ring16):
    """qe_propose (flags 1: appendEntry alone) and its instrumented variant:
    stages A and B of the wave's next tile are loaded before this tile's
    stores."""
    under_plans(eng, WALK, lambda trace: propose_vs_oracle(eng, S, F, masks, extras, max_cc,
                                                           max_ents, 1, ring16, G=G_WALK,
                                                           trace=trace))


#                S  F  masks           max_ents ring16
SWITCH_CASES = [(5, 8, ("inc",),       0,       False),
                (5, 8, ("inc", "out"), 2,       False),
                (9, 5, ("inc", "out"), 2,       True)]
SWITCH_IDS = ["masked", "joint", "ring16"]


@pytest.mark.parametrize("S,F,masks,max_ents,ring16", SWITCH_CASES, ids=SWITCH_IDS)
@pytest.mark.parametrize("all_groups", [False, True])
def test_switch_config_waves_walk(eng, S, F, masks, max_ents, ring16, all_groups):
    """qe_switch_config loads the header of the wave's next tile before this
    tile's stores and consumes it in the next iteration; with all_groups False
    the header's `switched` flag differs from lane to lane and from tile to
    tile."""
    under_plans(eng, WALK, lambda trace: switch_vs_oracle(eng, S, F, masks, max_ents, all_groups,
                                                          ring16, G=G_WALK, trace=trace))


@pytest.mark.parametrize("S,F,masks,max_ents,ring16", SWITCH_CASES, ids=SWITCH_IDS)
@pytest.mark.parametrize("all_groups", [False, True])
def test_switch_config_persistent_grid(eng, S, F, masks, max_ents, ring16, all_groups):
    """The same on the persistent grid: every wave consumes one or two
    prefetched headers, the last of them a ragged tile's."""
    G = persistent_groups()
    under_plans(eng, PERSISTENT, lambda trace: switch_vs_oracle(eng, S, F, masks, max_ents,
                                                                all_groups, ring16, G=G,
                                                                trace=trace))


@pytest.mark.parametrize("S,F,masks,max_ents,reads,ring16", [
    (5, 8, (), 0, True, False), (5, 32, ("inc", "out"), 2, False, False),
    (5, 8, ("inc",), 1, True, True)], ids=["reads", "no-reads", "ring16"])
def test_become_leader_waves_walk(eng, S, F, masks, max_ents, reads, ring16):
    under_plans(eng, WALK, lambda trace: become_leader_vs_oracle(eng, S, F, masks, max_ents, reads,
                                                                 ring16, G=G_WALK, trace=trace))
