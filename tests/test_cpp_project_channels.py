"""The C++ mirror's directional projection (bindings/cpp/hare.hpp: HistProjectChannels) through
bindings/cpp/project_channels_example.cpp, in the manner of tests/test_cpp_project.py: it compiles without a warning and its size checks
refuse; on a GPU its sums are the Python call's on the same scene, word for word, and its column of channel 0 is HistProject's."""
import os
import subprocess

import numpy as np
import pytest

import hare_amd as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_BINS, B, J, C = 16, 8, 3, 4


def build(tmp_path):
    exe = str(tmp_path / "hare_project_channels")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "bindings", "cpp"), os.path.join(ROOT, "bindings", "cpp", "project_channels_example.cpp"),
                           "-L", os.path.join(ROOT, "hare_amd"), "-lhare_hip", "-Wl,-rpath," + os.path.join(ROOT, "hare_amd"),
                           "-o", exe])
    return exe


def coef():
    i = np.arange(N_BINS)
    return np.stack([np.ones(N_BINS, np.int64), i, -1000 * (i + 1)]).astype(np.int32)


def test_cpp_project_channels_size_checks(tmp_path, gpu_available):
    r = subprocess.run([build(tmp_path)], capture_output=True, text=True)
    c = coef().reshape(-1)
    assert f"coef {c.size}: {c[0]} {c[-1]}" in r.stdout, r.stdout + r.stderr
    assert "refused 3" in r.stdout
    if not gpu_available:
        assert r.returncode == 2 and "no HIP device visible" in r.stdout and "project_channels:" not in r.stdout


@pytest.mark.gpu
def test_cpp_project_channels_on_gpu_matches_the_python_call(tmp_path):
    r = subprocess.run([build(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"project_channels: proj {2 * B * J * C * 2}, agree 1" in r.stdout, r.stdout
    c = np.array([[0, 0, 0], [2, 0, 0], [2, 2, 0], [0, 2, 0], [0, 0, 2], [2, 0, 2], [2, 2, 2], [0, 2, 2]], np.float64)
    f = [[0, 1, 2], [0, 2, 3], [4, 6, 5], [4, 7, 6], [0, 5, 1], [0, 4, 5], [3, 2, 6], [3, 6, 7], [0, 3, 7], [0, 7, 4], [1, 5, 6], [1, 6, 2]]
    verts = np.zeros((12, 4, 3))
    verts[:, :3] = c[np.array(f)]
    top = [H.Topology(verts, np.full(12, 3, np.int32)) for _ in range(2)]
    g = H.Voxel_Grid(top, 4)
    g.set_receivers([[1.0, 0.75, 0.5], [0.5, 0.5, 0.5]], [0.25, 0.125])
    g.set_absorption(np.full((12, 8), 0.25), top_index=1)
    rays = np.zeros((6, 6))
    rays[:, :3] = [1.0, 0.75, 0.5]
    for k in range(6):
        rays[k, 3 + k // 2] = -1.0 if k & 1 else 1.0
    hist = g.Receive_batch(rays, 3, N_BINS, 0.5, frac_bits=20, top_index=1, directional=True)[0]
    proj = g.hist_project_channels(hist, coef(), weight=H.air_weights([0.1] * B, 0.5, N_BINS))
    assert proj.shape == (2, B, J, C, 2) and proj[:, :, 0, 0].any() and proj[:, :, :, 1:].any()
    line = [l for l in r.stdout.splitlines() if l.startswith("proj:")][0]
    assert [int(x) for x in line.split()[1:]] == proj.reshape(-1).tolist()
