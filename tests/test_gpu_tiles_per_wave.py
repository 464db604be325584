"""qe_tune("tiles_per_wave") on the three chunked Progress-side launchers:
qe_progress_send, qe_check_quorum and qe_confchange give each wave a chunk of
tiles (etcd_amd/csrc/qe_launch.hpp); an override is floored at 2 and clamped
to the kernel's 8.  Whatever the chunk, the outputs and the state are the
same bits, and they are the oracle's."""
import copy

import numpy as np
import pytest
import torch

from oracle import confchange_ref as cc
from oracle import orc
from tests.test_gpu_confchange import run_differential
from tests.test_gpu_progress import DEV, EXTRAS, assert_same, random_state, to_dev_mask, to_device

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
