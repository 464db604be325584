"""bench.py's command line (CPU only): a plain run times the chosen workload
alone, --full adds the secondary workloads and the CPU baseline, and
--dump-outputs writes exact float32 / float64 copies of the outputs within
its size budget, the same elements on every run."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

bench = importlib.import_module("bench")


def test_parse_defaults_are_the_plain_run():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"


def _run_main(monkeypatch, capsys, argv):
    calls = []
    res = {"value": 1.0, "unit": "group-evals/s", "ms_per_step": 2.0, "groups_per_gpu": 64,
           "achieved_GBs": 1.0, "hbm_frac": 0.1, "kernel_ms": 2.0, "bytes_per_unit": 51,
           "invariant_violations": 0, "checksum": 5, "desc": "d"}

    def run_workload(name, args, d, steps, warmup, dump=None):
        calls.append(("run", name, steps, warmup, dump))
        return dict(res)

    monkeypatch.setattr(bench, "run_workload", run_workload)
    monkeypatch.setattr(bench, "config1", lambda a, d: calls.append(("config1",)) or {})
    monkeypatch.setattr(bench, "pcie_inclusive", lambda a, d: calls.append(("pcie",)) or {})
    monkeypatch.setattr(bench, "cpu_baseline", lambda a: calls.append(("cpu",)) or {"value": 0.5})
    monkeypatch.setattr("sys.argv", ["bench.py"] + argv)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 0
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return calls, json.loads(lines[0])


def test_plain_run_times_the_headline_alone(monkeypatch, capsys):
    calls, line = _run_main(monkeypatch, capsys, ["--gpus", "1", "--steps", "7", "--warmup", "2",
                                                  "--dump-outputs", "outdir"])
    assert calls == [("run", "config2_n5", 7, 2, "outdir")]
    assert line["aux"] == {} and line["cpu_baseline"] is None and line["vs_baseline"] is None
    assert line["steps"] == 7 and line["warmup"] == 2 and line["ms_per_step"] == 2.0
    for k in ("metric", "value", "unit", "higher_is_better", "dtype"):
        assert k in line


def test_full_run_adds_aux_and_cpu_baseline(monkeypatch, capsys):
    calls, line = _run_main(monkeypatch, capsys, ["--gpus", "1", "--steps", "8", "--warmup", "2",
                                                  "--full"])
    assert calls[0] == ("run", "config2_n5", 8, 2, None)
    assert ("config1",) in calls and ("pcie",) in calls and ("cpu",) in calls
    ran = {c[1] for c in calls if c[0] == "run"}
    assert ran == set(bench.WORKLOADS)
    assert set(line["aux"]) == (set(bench.WORKLOADS) - {"config2_n5"}) | {"config1_n3",
                                                                          "config2_n5_pcie"}
    assert line["cpu_baseline"] == {"value": 0.5} and line["vs_baseline"] == 2.0
    # the switches of the full run still take its parts out
    calls, line = _run_main(monkeypatch, capsys, ["--full", "--no-aux", "--no-cpu-baseline"])
    assert [c[0] for c in calls] == ["run"] and line["aux"] == {}


def test_dump_arrays_are_exact():
    u = np.array([0, 1, (1 << 63) + 12345, (1 << 64) - 1, (1 << 53) + 1], np.uint64)
    d = bench._dump_arrays("commit", u.view(np.int64))
    assert set(d) == {"commit_hi32", "commit_lo32"}
    assert all(a.dtype == np.float64 for a in d.values())
    back = (d["commit_hi32"].astype(np.uint64) << np.uint64(32)) | d["commit_lo32"].astype(np.uint64)
    assert np.array_equal(back, u)
    i32 = np.array([-(1 << 31), (1 << 31) - 1, 16777217], np.int32)
    d = bench._dump_arrays("ctx", i32)
    assert d["ctx"].dtype == np.float64 and np.array_equal(d["ctx"].astype(np.int32), i32)
    for a in (np.arange(256, dtype=np.uint8), np.array([-32768, 32767], np.int16)):
        d = bench._dump_arrays("m", a)
        assert d["m"].dtype == np.float32 and np.array_equal(d["m"].astype(a.dtype), a)


def test_dump_outputs_budget_and_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 1 << 16)
    n = 100_003
    commit = (torch.arange(n, dtype=torch.int64) * 0x9E3779B97F4A7C15) ^ (1 << 62)
    vote = (torch.arange(n) % 3).to(torch.uint8)
    small = torch.arange(17, dtype=torch.int16)
    outs = {"commit": commit, "vote": vote, "small": small, "absent": None}
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, outs)
    bench.dump_outputs(b, {k: (None if v is None else v.clone()) for k, v in outs.items()})
    names = sorted(os.listdir(a))
    assert names == ["commit_hi32.npy", "commit_lo32.npy", "small.npy", "vote.npy"]
    assert sum(os.path.getsize(os.path.join(a, f)) for f in names) <= (1 << 16) + 128 * len(names)
    k = 1 << 11  # the largest power of two with 20 k + 68 <= 65536
    pos = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, n, k))
    for f in names:
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y)
    assert np.array_equal(np.load(os.path.join(a, "vote.npy")), vote.numpy()[pos])
    assert np.array_equal(np.load(os.path.join(a, "small.npy")), small.numpy())
    lo = np.load(os.path.join(a, "commit_lo32.npy")).astype(np.uint64)
    hi = np.load(os.path.join(a, "commit_hi32.npy")).astype(np.uint64)
    assert np.array_equal((hi << np.uint64(32)) | lo, commit.numpy().view(np.uint64)[pos])
    # another rank of a multi-rank run writes beside rank 0's files
    bench.dump_outputs(a, {"vote": vote}, rank=1, world=2)
    assert os.path.exists(os.path.join(a, "vote.rank1.npy"))
