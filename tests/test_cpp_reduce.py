"""The C++ mirror's reduction calls (bindings/cpp/hare.hpp: HistReduce, ReceiveReduced, AirWeights, DecayLevel) through
bindings/cpp/reduce_example.cpp, in the manner of tests/test_cpp_receivers.py: it compiles without a warning, its helpers give the Python
helpers' values and its size checks refuse; on a GPU its sums and crossings are the Python call's on the same scene."""
import os
import subprocess

import numpy as np
import pytest

import hare_amd as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_BINS, B = 16, 8


def build(tmp_path):
    exe = str(tmp_path / "hare_reduce")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "bindings", "cpp"), os.path.join(ROOT, "bindings", "cpp", "reduce_example.cpp"),
                           "-L", os.path.join(ROOT, "hare_amd"), "-lhare_hip", "-Wl,-rpath," + os.path.join(ROOT, "hare_amd"),
                           "-o", exe])
    return exe


def spec():
    return dict(windows=[(0, N_BINS), (0, 2), (2, N_BINS)], levels=H.decay_levels([-5, -10]).tolist() + [0],
                weight=H.air_weights([0.1] * B, 0.5, N_BINS))


def test_cpp_reduce_helpers_and_size_checks(tmp_path, gpu_available):
    r = subprocess.run([build(tmp_path)], capture_output=True, text=True)
    s = spec()
    w = s["weight"].reshape(-1)
    assert f"levels {s['levels'][0]} {s['levels'][1]}, weight {w.size}: {w[0]} {w[-1]}" in r.stdout, r.stdout + r.stderr
    assert "refused 3" in r.stdout
    if not gpu_available:
        assert r.returncode == 2 and "no HIP device visible" in r.stdout and "reduce:" not in r.stdout


@pytest.mark.gpu
def test_cpp_reduce_on_gpu_matches_the_python_call(tmp_path):
    r = subprocess.run([build(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"reduce: sums {2 * B * 3 * 4}, cross {2 * B * 3}, agree 1" in r.stdout, r.stdout
    c = np.array([[0, 0, 0], [2, 0, 0], [2, 2, 0], [0, 2, 0], [0, 0, 2], [2, 0, 2], [2, 2, 2], [0, 2, 2]], np.float64)
    f = [[0, 1, 2], [0, 2, 3], [4, 6, 5], [4, 7, 6], [0, 5, 1], [0, 4, 5], [3, 2, 6], [3, 6, 7], [0, 3, 7], [0, 7, 4], [1, 5, 6], [1, 6, 2]]
    verts = np.zeros((12, 4, 3))
    verts[:, :3] = c[np.array(f)]
    T = [H.Topology(verts, np.full(12, 3, np.int32)) for _ in range(2)]
    g = H.Voxel_Grid(T, 4)
    g.set_receivers([[1.0, 0.75, 0.5], [0.5, 0.5, 0.5]], [0.25, 0.125])
    g.set_absorption(np.full((12, 8), 0.25), top_index=1)
    rays = np.zeros((6, 6))
    rays[:, :3] = [1.0, 0.75, 0.5]
    for k in range(6):
        rays[k, 3 + k // 2] = -1.0 if k & 1 else 1.0
    sums, cross, *_ = g.Receive_batch_reduced(rays, 3, N_BINS, 0.5, frac_bits=20, top_index=1, **spec())
    assert sums.any() and cross.any()
    lines = dict(l.split(":", 1) for l in r.stdout.splitlines() if l.startswith(("sums:", "cross:")))
    assert [int(x) for x in lines["sums"].split()] == sums.reshape(-1).tolist()
    assert [int(x) for x in lines["cross"].split()] == cross.reshape(-1).tolist()
