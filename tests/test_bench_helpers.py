"""bench.py's plumbing on the CPU: --steps split over --regions, the --dump-outputs writer (dtypes, seeded samples, size budget) and a
--dry-run --dump-outputs run end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_region_sizes_sum_to_steps():
    for steps in range(1, 60):
        for regions in range(1, 9):
            sizes = bench.region_sizes(steps, regions)
            assert sum(sizes) == steps
            assert len(sizes) == min(regions, steps)
            assert max(sizes) - min(sizes) <= 1 and min(sizes) >= 1


def test_dump_outputs_dtypes_and_files(tmp_path):
    d = str(tmp_path / "out")
    bench.dump_outputs(d, {"f64": torch.arange(4, dtype=torch.float64) / 3, "f32": torch.ones(2, 3), "bf16": torch.full((5,), 1.5, dtype=torch.bfloat16),
                           "i64": torch.tensor([1, 50256])})
    assert sorted(os.listdir(d)) == ["bf16.npy", "f32.npy", "f64.npy", "i64.npy"]
    a = np.load(os.path.join(d, "f64.npy"))
    assert a.dtype == np.float64 and np.array_equal(a, np.arange(4) / 3)
    assert np.load(os.path.join(d, "f32.npy")).shape == (2, 3)
    assert np.load(os.path.join(d, "bf16.npy")).dtype == np.float32 and np.all(np.load(os.path.join(d, "bf16.npy")) == 1.5)
    i = np.load(os.path.join(d, "i64.npy"))
    assert i.dtype == np.float32 and i.tolist() == [1.0, 50256.0]


def test_dump_outputs_refuses_more_than_the_budget(tmp_path):
    with pytest.raises(RuntimeError, match="budget"):
        bench.dump_outputs(str(tmp_path / "big"), {"x": torch.zeros(bench.DUMP_BYTES // 4 + 1)})
    assert not os.path.exists(tmp_path / "big")          # nothing written when over budget


def test_dump_sample_is_fixed_and_seeded():
    t = torch.arange(bench.DUMP_SAMPLE * 3, dtype=torch.float32)
    a, b = bench.dump_sample(t, 7), bench.dump_sample(t.clone(), 7)
    assert a.numel() == bench.DUMP_SAMPLE and torch.equal(a, b)
    assert torch.all(a[1:] > a[:-1])                      # sorted, no repeats
    assert not torch.equal(a, bench.dump_sample(t, 8))
    small = torch.arange(10.0)
    assert torch.equal(bench.dump_sample(small, 7), small)


def test_dry_run_dump_outputs_and_exact_steps(tmp_path):
    env = dict(os.environ, CC_BENCH_DRY_EXTRAS_S="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    d = str(tmp_path / "dump")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--dry-run", "--steps", "7", "--warmup", "1",
                          "--regions", "3", "--no-roofline-pass", "--dump-outputs", d], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    j = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert j["steps"] == 7 and j["timed_regions"]["steps_per_region"] == [3, 2, 2]
    assert os.listdir(d) == ["loss.npy"] and np.load(os.path.join(d, "loss.npy")).tolist() == [1.0]
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-run", "--steps", "0"], env=env, capture_output=True, text=True,
                         timeout=300)
    assert bad.returncode != 0 and "--steps" in bad.stderr


def test_plain_run_prints_the_headline_only_and_full_adds_the_extras():
    """A plain run sets up, warms up, times its steps and prints the headline line.  What takes runs of its own (N > 1: the steps without
    the all-reduce; the event-bracketed roofline steps) and rank 0's extras (sub-benches, CPU baselines) run only under --full."""
    env = dict(os.environ, CC_BENCH_DRY_EXTRAS_S="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    lines = {}
    for flags in ([], ["--full"]):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run", "--steps", "5", "--warmup", "1",
                              "--regions", "2"] + flags, env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        js = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        assert len(js) == 1, out.stdout[-2000:]
        lines[bool(flags)] = json.loads(js[0])
    plain, full = lines[False], lines[True]
    for j in (plain, full):
        assert j["n_gpus"] == 2 and j["steps"] == 5 and j["warmup"] == 1 and j["timed_regions"]["steps_per_region"] == [3, 2]
        assert j["unit"] == "samples/s" and j["higher_is_better"] is True and j["dtype"] == "bf16" and j["value"] > 0 and j["ms_per_step"] > 0
    extras = {"allreduce_exposed_ms", "exposed_allreduce_ms", "roofline", "roofline_lmhead", "cpu_baseline"}
    assert not extras & plain.keys(), sorted(extras & plain.keys())
    assert extras <= full.keys(), sorted(extras - full.keys())
    assert plain.keys() <= full.keys() and plain["metric"] == full["metric"]
