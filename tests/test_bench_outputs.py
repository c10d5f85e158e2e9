"""bench.py --dump-outputs and --full (CPU).

* dump_outputs writes every table as <name>.npy, float32 scores and float64 best densities, over one seeded sample of
  the frame columns -- the same columns in every table and in every run -- within DUMP_BYTES in all.
* Without --full a run prints the headline line alone: the N > 1 orchestration (RASR_BENCH_FENCE_PROBE, as
  tests/test_bench_fence.py) starts no fenced check."""
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _tables(rows, cols):
    s = torch.arange(rows * cols, dtype=torch.float32).reshape(rows, cols) / 7
    b = (torch.arange(rows * cols, dtype=torch.int64).reshape(rows, cols) % 160).to(torch.int32)
    return s, b


def test_dump_is_a_seeded_column_sample_within_the_budget(tmp_path, monkeypatch):
    rows, cols = 37, 1000
    monkeypatch.setattr(bench, "DUMP_BYTES", rows * 12 * 101 + 5)  # room for 101 columns of scores + best
    s, b = _tables(rows, cols)
    bench.dump_outputs(str(tmp_path / "a"), {"scores": s, "best": b})
    bench.dump_outputs(str(tmp_path / "b"), {"scores": s.clone(), "best": b.clone()})
    sa, ba = np.load(tmp_path / "a" / "scores.npy"), np.load(tmp_path / "a" / "best.npy")
    assert sa.dtype == np.float32 and ba.dtype == np.float64
    assert sa.shape == ba.shape == (rows, 101)
    assert sa.nbytes + ba.nbytes <= bench.DUMP_BYTES
    assert np.array_equal(sa, np.load(tmp_path / "b" / "scores.npy"))
    assert np.array_equal(ba, np.load(tmp_path / "b" / "best.npy"))
    # the sampled columns: distinct, ascending, the same in both tables, values untouched
    idx = np.rint(sa[0] * 7).astype(np.int64)
    assert (np.diff(idx) > 0).all() and idx.min() >= 0 and idx.max() < cols
    assert np.array_equal(sa, s.numpy()[:, idx])
    assert np.array_equal(ba, b.numpy()[:, idx].astype(np.float64))


def test_dump_small_table_whole_and_scores_only(tmp_path):
    s, _ = _tables(5, 64)
    bench.dump_outputs(str(tmp_path), {"scores": s, "best": None})
    assert sorted(os.listdir(tmp_path)) == ["scores.npy"]
    assert np.array_equal(np.load(tmp_path / "scores.npy"), s.numpy())


def test_plain_run_prints_the_headline_alone():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "RASR_BENCH_INJECT")}
    env["RASR_BENCH_FENCE_PROBE"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "0"],
                       capture_output=True, text=True, env=env, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["steps"] == 2 and line["value"] == 1.0 and "ms_per_step" in line
    for key in ("density_sharded", "density_sharded_capi", "modes", "small_batches", "drop_in_protocol",
                "host_boundary_all_ranks", "deadline"):
        assert key not in line, key
    assert line["cpu_baseline"] is None and line["host_boundary"] is None
