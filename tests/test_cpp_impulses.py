"""The C++ mirror's impulse calls (bindings/cpp/hare.hpp: SourcePaths, HistImpulses) through bindings/cpp/impulses_example.cpp, in the
manner of tests/test_cpp_decode.py: it compiles without a warning and its size checks refuse; on a GPU its peak is the Python calls' and
the numpy restatement's (tests/impulse_ref.py) on the same scene: the direct sound of receiver 0, at the sample of its distance."""
import os
import subprocess

import numpy as np
import pytest

import hare_amd as H
from tests.impulse_ref import impulse_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    exe = str(tmp_path / "hare_impulses")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "bindings", "cpp"), os.path.join(ROOT, "bindings", "cpp", "impulses_example.cpp"),
                           "-L", os.path.join(ROOT, "hare_amd"), "-lhare_hip", "-Wl,-rpath," + os.path.join(ROOT, "hare_amd"),
                           "-o", exe])
    return exe


def test_cpp_impulses_size_checks(tmp_path, gpu_available):
    r = subprocess.run([build(tmp_path)], capture_output=True, text=True)
    assert "refused 4" in r.stdout, r.stdout + r.stderr
    if not gpu_available:
        assert r.returncode == 2 and "no HIP device visible" in r.stdout and "impulses:" not in r.stdout


@pytest.mark.gpu
def test_cpp_impulses_on_gpu_matches_the_python_calls_and_the_reference(tmp_path):
    r = subprocess.run([build(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    L = (5.0, 4.0, 3.0)
    c = np.array([(0, 0, 0), (L[0], 0, 0), (L[0], L[1], 0), (0, L[1], 0), (0, 0, L[2]), (L[0], 0, L[2]), (L[0], L[1], L[2]), (0, L[1], L[2])], np.float64)
    f = [(0, 1, 2), (0, 2, 3), (4, 6, 5), (4, 7, 6), (0, 5, 1), (0, 4, 5), (3, 2, 6), (3, 6, 7), (0, 3, 7), (0, 7, 4), (1, 5, 6), (1, 6, 2)]
    verts = np.zeros((12, 4, 3))
    for p, tri in enumerate(f):
        verts[p, :3] = c[list(tri)]
    g = H.Voxel_Grid([H.Topology(verts, np.full(12, 3, np.int32))], 4)
    g.set_receivers(np.array([[3.5, 2.5, 1.5], [1.0, 3.0, 2.0]]), np.array([0.25, 0.25]))
    g.set_absorption(np.full((12, 2), 0.25))
    g.set_source((1.5, 1.0, 1.25), power=[1.0, 0.5])
    n_bins, bin_len = 2048, 343.0 / 48000.0
    hist, _ = g.Source_paths(1 << 20, n_bins, bin_len, frac_bits=40)
    taps = np.array([[0.25, 0.5, 0.25], [-0.25, 0.5, -0.25]])
    out = g.hist_impulses(hist, taps, 40, 1, n_bins)
    assert out.tobytes() == impulse_ref(hist, taps, 40, 1, n_bins).tobytes()
    peak = int(np.argmax(np.abs(out[0, 0])))
    dist = float(np.linalg.norm(np.array([3.5, 2.5, 1.5]) - np.array([1.5, 1.0, 1.25])))
    assert peak == int(dist / bin_len)                                   # the direct sound, in the sample it arrives in
    line = [l for l in r.stdout.splitlines() if l.startswith("impulses:")][0]
    assert f"entries {int((hist != 0).sum())}, out {out.size}, receiver 0 peak at sample {peak} " in line, line
    assert float(line.split()[-1]) == out[0, 0, peak]
