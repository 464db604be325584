"""bench.py --dump-outputs on the GPU: one plain run of the headline workload
at a small size writes its last step's CommittedIndex / VoteResult, and the
files equal the oracle's results for the same generated groups (the odd
group count is below the sample size, so every group is written)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_the_last_steps_outputs(tmp_path, orc):
    G, S = 100_003, 5
    out = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps",
                        "3", "--warmup", "1", "--groups", str(G), "--dump-outputs", out],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    assert line["aux"] == {} and line["cpu_baseline"] is None
    assert sorted(os.listdir(out)) == ["commit_hi32.npy", "commit_lo32.npy", "vote.npy"]
    hb = orc.Batch(G, S, masks=())
    orc.gen_batch(hb, 0x5EED)
    commit, vote = orc.commit_vote(hb)[:2]
    hi = np.load(os.path.join(out, "commit_hi32.npy"))
    lo = np.load(os.path.join(out, "commit_lo32.npy"))
    v = np.load(os.path.join(out, "vote.npy"))
    assert hi.dtype == lo.dtype == np.float64 and v.dtype == np.float32
    assert np.array_equal((hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64), commit)
    assert np.array_equal(v.astype(np.uint8), vote)
