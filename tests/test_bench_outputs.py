"""bench.py's options on CPU: --steps / --full checks and what --dump-outputs writes (the GPU run that dumps a real step is in
tests/test_gpu_bench.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
import hare_amd as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _events(n):
    ev = np.zeros(n, H.capi.XEVENT_DTYPE)
    rng = np.random.default_rng(3)
    ev["hit"] = rng.integers(0, 2, n)
    ev["poly_id"] = np.where(ev["hit"] != 0, rng.integers(0, 1_000_000, n), -1)
    for f in ("t", "x", "y", "z", "u", "v"):
        ev[f] = rng.standard_normal(n)
    return ev


@pytest.mark.parametrize("argv,msg", [
    (["--steps", "0"], "--steps must be >= 1"),
    (["--extra-configs"], "--extra-configs is measured by --full"),
    (["--inproc-scenes", "2"], "--inproc-scenes is measured by --full"),
    (["--bounces", "8", "--bounce-api", "batch"], "--bounce-api batch is measured by --full"),
])
def test_bench_refuses_options_it_would_not_honour(argv, msg):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and msg in r.stderr, r.stderr


def test_bench_full_options_parse():
    a = bench.parse_args(["--full", "--extra-configs", "--inproc-scenes", "2", "--steps", "7", "--dump-outputs", "d"])
    assert a.full and a.extra_configs and a.inproc_scenes == 2 and a.steps == 7 and a.dump_outputs == "d"
    assert not bench.parse_args([]).full and bench.parse_args([]).dump_outputs is None


def test_dump_writes_every_field_of_a_whole_batch(tmp_path):
    ev = _events(1000)
    bench.write_outputs(str(tmp_path), ev, 1000, int(ev["hit"].sum()))
    assert sorted(os.listdir(tmp_path)) == sorted(f"{f}.npy" for f in ("counters", "shard", "hit", "poly_id", "t", "x", "y", "z", "u", "v"))
    for f in ("hit", "poly_id", "t", "x", "y", "z", "u", "v"):
        a = np.load(tmp_path / f"{f}.npy")
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, ev[f]), f
    assert np.load(tmp_path / "counters.npy").tolist() == [1000, int(ev["hit"].sum())]
    assert np.load(tmp_path / "shard.npy").tolist() == [0, 1000, 1]                  # one rank: the whole burst
    bench.write_outputs(str(tmp_path), ev[:500], 1000, int(ev["hit"].sum()), shard=(500, 500, 2))
    assert np.load(tmp_path / "shard.npy").tolist() == [500, 500, 2]                 # rank 0 of two would be (0, 500, 2): the rays are named


def test_dump_of_a_large_batch_is_a_fixed_sample_within_64_mb(tmp_path):
    n = 1_300_000                   # 56 B of fields per ray: more than 64 MB
    ev = _events(n)
    for d in ("a", "b"):
        bench.write_outputs(str(tmp_path / d), ev, n, 0)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 64_000_000
    idx = np.load(tmp_path / "a" / "ray_index.npy").astype(np.int64)
    assert len(idx) > 900_000 and np.all(np.diff(idx) > 0) and idx[-1] < n
    assert np.array_equal(np.load(tmp_path / "a" / "t.npy"), ev["t"][idx])
    for f in os.listdir(tmp_path / "a"):                 # the same sample every time
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f
    bench.write_outputs(str(tmp_path / "a"), ev[:1000], 1000, 0)      # a whole batch into the same folder: no stale sample index
    assert not (tmp_path / "a" / "ray_index.npy").exists()
